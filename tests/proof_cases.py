"""What the planner PROVES on the host, as tables and graph recipes (plain data: importable without a GPU), shared by
tests/test_proofs_sim.py (CPU: the oracle, the host-logic simulator, the matcher through tests/cpp/voice_proof.cpp) and
tests/test_hip_proofs.py (MI355X).  A proof that is wrong for one input makes a correct kernel give a wrong sample, so every
table row comes with the input that would show it.

MOD1_DIVIDENDS    the sign rule (match.cpp fract_form_is_exact): a 32-leaf voice whose leaf k is 2^-(k+1) * Modulo(D, 1).  The
                  generated kernel may replace that Modulo by one v_fract_f32 for a whole wave when fast_ok is true and the wave's
                  inputs are in [+0, 2^32]; that is exact only if D is then finite and >= +0 (never -0).
                    FAST  fast_ok must be true
                    NOT   a witness input in [+0, 2^32] makes D negative, -0, NaN or infinite: fast_ok must be false
                    FREE  D is in fact always finite and >= +0, but the rule may refuse it: recorded, not pinned (four rows, no more)
PLANTED           one value out of [+0, 2^32] in one lane of an otherwise in-range call: the per-wave vote must see it.
BOUNDED_AMOUNTS   Delay(Multiply(In0, 0.5), A) with A read from In1 and an interval whose top the amount ATTAINS.
SPIKE_*           observed hulls (FR_DELAY_OBSERVED): rows of +0 with one spike, at the edges of input_range_kernel's lanes, waves,
                  blocks and grid-stride passes.

Expressions are tuples: ("in", slot), ("c", value), ("col", values per leaf) and (op, a, b) with op one of prim_pairs.OPS;
`evaluate` computes one with prim_pairs.reference (float64, rounded once per op), `build` makes its nodes for P leaves."""
import numpy as np

import prim_pairs as pp
import stage_variants as sv
from libfriendship_amd import synth
from stage_reference import Graph

F = np.float32
P = 32
TWO32 = F(4294967296.0)
X, Y = ("in", 0), ("in", 1)
W_COL = (F(0.0013) * np.arange(1, P + 1, dtype=np.float32)).astype(np.float32)      # w_k = 0.0013 * (k + 1)
W = ("col", W_COL)
SCALE = ("col", pp.leaf_scales(P))
ONE = ("c", F(1.0))
WATCHED = (0, 7, 31)                                                                # the leaves whose D the oracle renders


def c(v):
    return ("c", F(v))


def col_with(k, v):
    w = W_COL.copy()
    w[k] = v
    return ("col", w)


def has_op(e, name):
    return e[0] == name or (e[0] in pp.OPS and (has_op(e[1], name) or has_op(e[2], name)))


def build(g, e, n=P):
    """The operand (for GraphArrays.binop) of expression e over n leaves."""
    if e[0] == "in":
        return synth.IN(e[1])
    if e[0] == "c":
        return synth.C(np.full(n, e[1], np.float32))
    if e[0] == "col":
        return synth.C(np.asarray(e[1], np.float32))
    return g.binop(pp.KIND[e[0]], build(g, e[1], n), build(g, e[2], n), n)


def evaluate(e, rows, k, semantics="reference"):
    """Expression e of leaf k on the input rows, by prim_pairs.reference."""
    if e[0] == "in":
        return np.asarray(rows[e[1]], np.float32)
    if e[0] == "c":
        return F(e[1])
    if e[0] == "col":
        return F(e[1][k])
    return pp.reference(e[0], evaluate(e[1], rows, k, semantics), evaluate(e[2], rows, k, semantics), semantics)


def leaf_of(D):
    return ("Multiply", SCALE, ("Modulo", D, ONE))


def voice_tree(leaf, n_voices=1, cols=None):
    """n_voices rows, each the balanced sum of P leaves `leaf`.  cols: {id(col expression): [n_voices, P] values} gives a "col" of
    the leaf other values per voice (voices that differ are not merged at lowering)."""
    g = synth.GraphArrays()
    n = n_voices * P

    def operand(e):
        if e[0] == "in":
            return synth.IN(e[1])
        if e[0] == "c":
            return synth.C(np.full(n, e[1], np.float32))
        if e[0] == "col":
            v = cols[id(e)] if cols and id(e) in cols else np.tile(np.asarray(e[1], np.float32), n_voices)
            return synth.C(np.asarray(v, np.float32).ravel())
        return g.binop(pp.KIND[e[0]], operand(e[1]), operand(e[2]), n)

    leaves = operand(leaf)
    roots = synth.sum_tree(g, leaves.reshape(n_voices, P))
    g.edge(roots, 0, 0, np.arange(n_voices, dtype=np.uint32))
    return g.finish(n_voices)


def dividend_rows_tree(D):
    """Output row i = D of leaf WATCHED[i], nothing else: what the oracle renders of D itself."""
    g = synth.GraphArrays()
    d = build(g, D)
    for row, k in enumerate(WATCHED):
        if isinstance(d, tuple) and d[0] == "in":
            g.edge(0, 0, d[1], row)
        else:
            g.edge(d[k], 0, 0, row)
    return g.finish(len(WATCHED))


# ---- MOD1_DIVIDENDS ---------------------------------------------------------------------------------------------------------------
def _row(name, D, cls, witness=None, semantics=None, options=None):
    """witness: (x, y) in [+0, 2^32] at which D offends.  semantics: both where D holds a Minimum (the only primitive the
    semantics part at), the reference's else; a row that is only one semantics' says so."""
    if semantics is None:
        semantics = pp.SEMANTICS if has_op(D, "Minimum") else pp.SEMANTICS[:1]
    return {"name": name, "D": D, "cls": cls, "witness": witness, "semantics": tuple(semantics), "options": dict(options or {})}


def _mul(a, b):
    return ("Multiply", a, b)


def _sum(a, b):
    return ("Sum2", a, b)


def _div(a, b):
    return ("Divide", a, b)


def _mod(a, b):
    return ("Modulo", a, b)


def _min(a, b):
    return ("Minimum", a, b)


XW = _mul(X, W)
XY = _mul(X, Y)
NAN = F(np.nan)
MOD1_DIVIDENDS = [
    _row("x", X, "FAST"),
    _row("x*w", XW, "FAST"),
    _row("x*w+0.25", _sum(XW, c(0.25)), "FAST"),
    _row("x*y", XY, "FAST"),
    _row("x*(+0)", _mul(X, c(0.0)), "FAST"),
    _row("x/4", _div(X, c(4.0)), "FAST"),
    _row("x/(y+1)", _div(X, _sum(Y, c(1.0))), "FAST"),
    _row("min(x,5)", _min(X, c(5.0)), "FAST"),
    _row("min(5,x)", _min(c(5.0), X), "FAST"),
    _row("mod(x,0.75)", _mod(X, c(0.75)), "FAST"),
    _row("mod(mod(x*w,1)+0.25,1)", _sum(_mod(XW, ONE), c(0.25)), "FAST"),
    _row("0.25+2*x,fma", _sum(c(0.25), _mul(c(2.0), X)), "FAST", options={"FR_JIT_FMA": "1"}),
    _row("0.25+2*x,nofma", _sum(c(0.25), _mul(c(2.0), X)), "FAST", options={"FR_JIT_FMA": "0"}),
    _row("x+(-0.5)", _sum(X, c(-0.5)), "NOT", (0.0, 0.0)),
    _row("x*(-0)", _mul(X, c(-0.0)), "NOT", (1.0, 0.0)),
    _row("x*3e38", _mul(X, c(3e38)), "NOT", (2.0, 0.0)),
    _row("x*inf", _mul(X, c(np.inf)), "NOT", (0.0, 0.0)),
    _row("(x*y)*(x*y)", _mul(XY, XY), "NOT", (TWO32, TWO32)),
    _row("x/(+0)", _div(X, c(0.0)), "NOT", (0.0, 0.0)),
    _row("x/(-2)", _div(X, c(-2.0)), "NOT", (1.0, 0.0)),
    _row("1/x", _div(ONE, X), "NOT", (0.0, 0.0)),
    _row("min(x,-1)", _min(X, c(-1.0)), "NOT", (0.0, 0.0)),
    _row("mod(x,+0)", _mod(X, c(0.0)), "NOT", (1.0, 0.0)),
    _row("mod(5,x)", _mod(c(5.0), X), "NOT", (0.0, 0.0)),
    _row("mod(x,y)", _mod(X, Y), "NOT", (1.0, 0.0)),
    _row("x*c,c7=-0", _mul(X, col_with(7, -0.0)), "NOT", (1.0, 0.0)),
    _row("x*c,c7=nan", _mul(X, col_with(7, np.nan)), "NOT", (1.0, 0.0)),
    _row("min(nan,x),sparkle", _min(c(NAN), X), "NOT", (1.0, 0.0), semantics=("sparkle",)),
    _row("x+(-0)", _sum(X, c(-0.0)), "FREE"),
    _row("mod(x,-0.75)", _mod(X, c(-0.75)), "FREE"),
    _row("min(x,nan)", _min(X, c(NAN)), "FREE"),
    _row("min(nan,x),reference", _min(c(NAN), X), "FREE", semantics=("reference",)),
]
N_FREE = 4


def mod1_items(cls):
    """[(row, semantics)] of a class: one generated kernel each."""
    return [(r, s) for r in MOD1_DIVIDENDS if r["cls"] == cls for s in r["semantics"]]


def chunks(items, n=6):
    return [items[i:i + n] for i in range(0, len(items), n)]


IN_RANGE_BASE = np.array([0.0, 1e-45, 0.5, 1.0, 2.0, 8388608.5, 16777216.0, 4294967296.0], np.float32)


def in_range_rows(n_random=256, seed=0x5EED0B01):
    """(x, y), every value in [+0, 2^32]: the base values crossed (64 frames), then seeded values of every magnitude up to 2^32."""
    m = synth.uniform01(seed, 2 * n_random)
    e = (synth.splitmix64(seed + 1, 2 * n_random) % np.uint64(40)).astype(np.float64) - 7.0
    r = np.minimum(m * 2.0 ** e, 4294967296.0).astype(np.float32)
    x = np.concatenate([np.repeat(IN_RANGE_BASE, len(IN_RANGE_BASE)), r[:n_random]])
    y = np.concatenate([np.tile(IN_RANGE_BASE, len(IN_RANGE_BASE)), r[n_random:]])
    assert (x.view(np.uint32) <= 0x4F800000).all() and (y.view(np.uint32) <= 0x4F800000).all()
    return x, y


def hostile_rows():
    x = pp.signal_row()
    return x, x[::-1].copy()


def offends(d):
    """Per sample: D is not what v_fract_f32 may take for fmod -- negative, -0, NaN or infinite."""
    d = np.asarray(d, np.float32)
    return ~np.isfinite(d) | ((d.view(np.uint32) >> 31) != 0)


# ---- one lane out of range ------------------------------------------------------------------------------------------------------
PLANT_T = 5 * 64 + 37
PLANT_VALUES = np.array([-0.0, -1e-30, -4.0, 4294967808.0, np.nan], np.float32)      # 4294967808 = the f32 above 2^32
PLANT_FRAMES = (2 * 64 + 0, 2 * 64 + 31, 2 * 64 + 32, 2 * 64 + 63, 0, PLANT_T - 1)   # lanes 0, 31, 32, 63 of wave 2; the call's ends
PLANT_VOICES = {
    "x*w": (leaf_of(XW), 1, (0,)),                                                   # (leaf, inputs the voice reads, the FRACT_INPUTS slots)
    "mod(x*w,1)*y": (_mul(SCALE, _mul(_mod(XW, ONE), Y)), 2, (0,)),
    "x*y*w": (leaf_of(_mul(XY, W)), 2, (0, 1)),
}


def plant_base_rows(T=PLANT_T, start=0):
    """In-range ramps: x = 0.25 + 0.37 * t, y = 1 + t / 128."""
    t = np.arange(start, start + T, dtype=np.float32)
    return [(F(0.25) + F(0.37) * t).astype(np.float32), (F(1.0) + t * F(1.0 / 128)).astype(np.float32)]


def plants(n_inputs):
    """(slot, frame, value) of every planted call."""
    return [(s, f, v) for s in range(n_inputs) for f in PLANT_FRAMES for v in PLANT_VALUES]


def fract_body_voice(x):
    """The voice x*w with EVERY Modulo(., 1) restated as a - floorf(a): what a wave computes that takes the fract body."""
    a = pp.reference("Multiply", np.asarray(x, np.float32)[:, None], W_COL[None, :])
    fr = (a - np.floor(a)).astype(np.float32)
    return pp.tree_sum(pp.reference("Multiply", pp.leaf_scales(P)[None, :], fr))


def multi_voices(T=PLANT_T, vpw0=8):
    """The smallest voice count for which csrc/bankplan.hpp whole_voices_per_wave takes 32-leaf voices whole (jit_bank_multi): from
    8 in a row, halved while the launch has fewer than 2048 workgroups, taken if it then has at least 1024."""
    tiles = (T + 63) // 64

    def vpw(voices):
        v = vpw0
        nb = lambda per: ((voices + 4 * per - 1) // (4 * per)) * tiles      # noqa: E731
        while v > 1 and nb(v) < 2048:
            v >>= 1
        return v if nb(v) >= 1024 else 0
    n = 1
    while not vpw(n):
        n += 1
    return n


def voice_cols(n_voices):
    """w per voice: w_k * (1 + v / 4096), so that no two voices are one node."""
    return (W_COL[None, :] * (F(1.0) + np.arange(n_voices, dtype=np.float32)[:, None] / F(4096.0))).astype(np.float32)


DELAYED_VOICE_FRAMES = 100
DELAYED_VOICE_START = 1000


def delayed_voice_tree(leaf, d=DELAYED_VOICE_FRAMES):
    """Row 0 = Delay(voice, d): the voice goes to a ring whose window starts d frames before the call."""
    g = synth.GraphArrays()
    root = synth.sum_tree(g, build(g, leaf).reshape(1, P))
    dl = g.binop(synth.K_DELAY, root, synth.C(np.array([d], np.float32)), 1)
    g.edge(dl, 0, 0, 0)
    return g.finish(1)


# ---- BOUNDED_AMOUNTS ----------------------------------------------------------------------------------------------------------------
IN1 = ("in", 1)
BOUNDED_AMOUNTS = [
    # (name, A, the largest trunc(A) the In1 row below reaches = the top of A's interval in frames)
    ("min(48,in1)", _min(c(48.0), IN1), 48),
    ("mod(in1,48)", _mod(IN1, c(48.0)), 48),                 # In1 = -1e-45: fmod gives -1e-45, + 48 rounds to exactly 48.0
    ("mod(in1,-7)", _mod(IN1, c(-7.0)), 6),                  # < 7; the negatives delay by 0 frames
    ("10+30*mod(in1,1)", _sum(c(10.0), _mul(c(30.0), _mod(IN1, ONE))), 40),
    ("min(90,mod(in1,128))/2", _div(_min(c(90.0), _mod(IN1, c(128.0))), c(2.0)), 45),
    ("0.5*min(90,mod(in1,128))", _mul(c(0.5), _min(c(90.0), _mod(IN1, c(128.0)))), 45),
    ("delay(mod(in1,48),3)", ("Delay", _mod(IN1, c(48.0)), c(3.0)), 48),
]
AMOUNT_DRIVERS = np.array([-1e-45, 6.5, 100.0, 127.5, 47.99, 0.99999994, 0.0, 48.0, 1e30, 6.9999995, -6.5, 90.0], np.float32)
AMOUNT_CALLS = (300, 217)


def amount_rows(n=sum(AMOUNT_CALLS), seed=0x5EED0B02):
    """[In0: finite noise, In1: stage_variants.HOSTILE_AMOUNTS and the values that drive every A to its top and its bottom]."""
    vals = np.concatenate([sv.HOSTILE_AMOUNTS, AMOUNT_DRIVERS])
    return [np.random.default_rng(seed).normal(size=n).astype(np.float32), np.resize(vals, n).astype(np.float32)]


def _stage(g, e):
    """Expression e (with ("Delay", a, b) allowed) as a node or leaf of a stage_reference.Graph."""
    if e[0] in ("in", "c"):
        return (e[0], float(e[1]) if e[0] == "c" else e[1])
    return g.op(e[0], _stage(g, e[1]), _stage(g, e[2]))


def bounded_delay_graph(A):
    g = Graph()
    g.output(g.op("Delay", g.op("Multiply", ("in", 0), ("c", 0.5)), _stage(g, A)), 0)
    return g


def amount_values(A, rows, semantics):
    """A per frame by prim_pairs.reference (a Delay in A by a whole constant: a shift, zeros before frame 0)."""
    if A[0] == "Delay":
        inner, d = amount_values(A[1], rows, semantics), int(A[2][1])
        return np.concatenate([np.zeros(d, np.float32), inner[:-d]])
    if A[0] in pp.OPS:
        return pp.reference(A[0], amount_values(A[1], rows, semantics), amount_values(A[2], rows, semantics), semantics)
    return np.broadcast_to(evaluate(A, rows, 0), np.shape(rows[0])).astype(np.float32)


def frames_of(amounts):
    """trunc(A) as the reference converts an amount that stays below 2^31: NaN and negatives are 0 frames."""
    a = np.asarray(amounts, np.float64)
    return np.where(np.isnan(a) | (a < 0), 0.0, np.floor(a)).astype(np.int64)


# The loop case.  The issue's amount, 3 + Modulo(In1, 5), is NaN for In1 = +inf or NaN -- a NaN amount delays by 0 frames, a
# loop without a delay -- so the planner must refuse it (FR_ERR_CYCLE); with the Modulo clamped by a constant on the LEFT of a
# Minimum the amount is in [3, 8] and never NaN, and In1 = 0 makes it 3: the proven lower bound (2 frames after the outward
# widening of 3 + 0) is reached to within the widening.
LOOP_DYN = {"FR_LOOP_DYN": "1"}


def dyn_loop_graph(clamped=True):
    """x = In0 + 0.5 * Delay(x, 3 + [Minimum(5,] Modulo(In1, 5) [)])"""
    g = Graph()
    x = g.node("Sum2")
    g.connect(("in", 0), x, 0)
    m = g.op("Modulo", ("in", 1), ("c", 5.0))
    amt = g.op("Sum2", ("c", 3.0), g.op("Minimum", ("c", 5.0), m) if clamped else m)
    g.connect(g.op("Multiply", g.op("Delay", x, amt), ("c", 0.5)), x, 1)
    g.output(x, 0)
    return g


def dyn_loop_rows(n=700, seed=0x5EED0B03):
    vals = np.concatenate([np.array([0.0, 0.0, 0.0, 4.9999995, 2.5, 1.0, -1e-45, 7.25, -3.0], np.float32), sv.HOSTILE_AMOUNTS])
    return [np.random.default_rng(seed).normal(size=n).astype(np.float32), np.resize(vals, n).astype(np.float32)]


# ---- observed hulls -------------------------------------------------------------------------------------------------------------------
OBSERVED = {"FR_DELAY_OBSERVED": "1"}
RANGE_BLOCK = 16384            # csrc/engine.cpp reduce_device_rows: a block per 16 K values, csrc/kernels.hpp RANGE_MAX_BLOCKS = 64 at most
SPIKE_LENGTHS = (1, 63, 64, 65, 255, 256, 257, RANGE_BLOCK, RANGE_BLOCK + 1)
SPIKE_LONGEST = 64 * RANGE_BLOCK + 257          # the grid-stride tail past 64 blocks
RANGE_MAX_ROWS = 32


def spike_positions(L):
    return sorted({p for p in (0, 63, 64, 255, 256, L - 1, RANGE_BLOCK - 1, RANGE_BLOCK) if 0 <= p < L})


def observed_delay_tree(n_delays=1):
    """Row j = Delay(Multiply(In0, 0.5), In(1 + j)): no voice, an amount nobody can bound but by observation."""
    g = synth.GraphArrays()
    src = g.binop(synth.K_MUL, synth.IN(0), synth.C(np.array([0.5], np.float32)), 1)
    for j in range(n_delays):
        dl = g.nodes(synth.K_DELAY, 1)
        g.edge(src, dl, 0, 0)
        g.edge(0, dl, 1 + j, 1)
        g.edge(dl, 0, 0, j)
    return g.finish(n_delays)


def spike_row(L, pos, value):
    r = np.zeros(L, np.float32)
    r[pos] = value
    return r


def source_row(L):
    """In0: t + 1, exact in f32 up to 2^24 frames (the Delay's output names the frame it read)."""
    return np.arange(1, L + 1, dtype=np.float32)
