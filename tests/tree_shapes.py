"""A matrix of Sum2-tree shapes for the schedule kernels (gbank_kernel, gbank_multi_kernel, bank_stream_general_kernel), a dense
f32 reference in each tree's OWN association, and an independent restatement of the schedule the matcher cuts a tree into.
Plain data and recipes: importable without a GPU.  tests/test_tree_shapes.py proves the reference and the table's claims on the
CPU; tests/test_hip_tree_shapes.py runs the table on the MI355X.

A SHAPE is written as nested pairs.  An integer k is a complete adjacent-pairs sub-tree of 2^k leaves (synth.sum_tree of a
power of two), a pair (a, b) is Sum2(a, b).  Two more forms make DAGs: same(s) is Sum2(x, x) with ONE node x of shape s (the
matcher walks it twice), shared(key, s) is a sub-tree of shape s that every voice of one graph naming `key` shares.  plain(shape)
is the tree that the values follow, with both forms expanded.

The engine (csrc/match.cpp emit_general) cuts a voice into ITEMS, the maximal complete sub-trees of at most 2^11 leaves, in
post-order, and counts per item the merges (v = pop() + v) that follow it; the kernels run that on a stack of 16 columns.
schedule_of restates it from the notation alone.  A voice is served as one general voice when its schedule needs at most 16
stack levels and it has at least 16 leaves; otherwise a stage program adds up what its operands are (serving_of).

The graph builder hash-conses nothing itself, but the engine's lowering orders the operands of a Sum2 by node id; in a tree every
left operand is lowered first, so the order of the notation is the order of the schedule.  Only shared(...) can meet an operand
that was lowered earlier: the table keeps a shared sub-tree on the left of the voice that comes second."""
import numpy as np

import bank_reference
from libfriendship_amd import synth

_F = np.float32
MAX_ITEM_LOG2 = 11      # items of at most 2048 leaves
MAX_DEPTH = 16          # the evaluation stack's columns
MIN_LEAVES = 16         # a smaller sum is a stage program
SEED = 0x5EED0A00


# ---- the notation ----------------------------------------------------------------------------------------------------------------

def same(s):
    return ("same", s)


def shared(key, s):
    return ("shared", key, s)


def plain(s):
    """The shape as nested pairs and integers only."""
    if isinstance(s, int):
        return s
    if s[0] == "same":
        p = plain(s[1])
        return (p, p)
    if s[0] == "shared":
        return plain(s[2])
    return (plain(s[0]), plain(s[1]))


def n_leaves(s):
    s = plain(s)
    return 1 << s if isinstance(s, int) else n_leaves(s[0]) + n_leaves(s[1])


def rchain(items):
    """(i0, (i1, (i2, ...)))"""
    s = items[-1]
    for x in reversed(items[:-1]):
        s = (x, s)
    return s


def lchain(items):
    """(((i0, i1), i2), ...)"""
    s = items[0]
    for x in items[1:]:
        s = (s, x)
    return s


def mirror(s):
    """Every pair with its operands the other way round."""
    return s if isinstance(s, int) else (mirror(s[1]), mirror(s[0]))


# ---- the schedule, restated ------------------------------------------------------------------------------------------------------

def _complete(s):
    """k if the plain shape s is a complete sub-tree of 2^k <= 2^11 leaves, else -1."""
    if isinstance(s, int):
        return s if s <= MAX_ITEM_LOG2 else -1
    a, b = _complete(s[0]), _complete(s[1])
    return a + 1 if a >= 0 and a == b and a < MAX_ITEM_LOG2 else -1


def _split(s):
    """An integer above 11 as pairs of halves (2^12 complete leaves are two items and a merge)."""
    if isinstance(s, int):
        return s if s <= MAX_ITEM_LOG2 else (_split(s - 1), _split(s - 1))
    return (_split(s[0]), _split(s[1]))


def schedule_of(shape):
    """{"items": [k], "merges": [merges after the item], "depth": most stack levels in use, "offsets": [first leaf of the item]}."""
    items, merges, offsets = [], [], []
    state = {"depth": 0, "max": 0, "pos": 0}

    def walk(s):
        k = _complete(s)
        if k >= 0:
            items.append(k)
            merges.append(0)
            offsets.append(state["pos"])
            state["pos"] += 1 << k
            state["depth"] += 1
            state["max"] = max(state["max"], state["depth"])
            return
        walk(s[0])
        walk(s[1])
        merges[-1] += 1
        state["depth"] -= 1

    walk(_split(plain(shape)))
    assert state["depth"] == 1 and sum(merges) == len(items) - 1
    return {"items": items, "merges": merges, "depth": state["max"], "offsets": offsets}


def served(shape):
    """One general voice: at most 16 stack levels, at least 16 leaves."""
    return schedule_of(shape)["depth"] <= MAX_DEPTH and n_leaves(shape) >= MIN_LEAVES


def serving_of(shape):
    """(leaf counts of the general voices the shape is served by, stage programs): a shape that is no voice is one program over
    whatever voices its operands are."""
    def voices(s):
        if served(s):
            return [n_leaves(s)]
        return [] if isinstance(s, int) else voices(s[0]) + voices(s[1])
    s = _split(plain(shape))
    return ([n_leaves(s)], 0) if served(s) else (voices(s), 1)


# ---- the dense reference ---------------------------------------------------------------------------------------------------------

def _eval(s, L, pos):
    """(values [v, T], next leaf) of the plain shape s over the leaves L [v, P, T] from leaf `pos` on."""
    if isinstance(s, int):
        cur = L[:, pos:pos + (1 << s)]
        with np.errstate(all="ignore"):
            while cur.shape[1] > 1:
                cur = cur[:, 0::2] + cur[:, 1::2]
        return cur[:, 0], pos + (1 << s)
    a, pos = _eval(s[0], L, pos)
    b, pos = _eval(s[1], L, pos)
    with np.errstate(all="ignore"):
        return a + b, pos


def render_shapes(shapes, w, amp, t, budget=1 << 22):
    """shapes: V shapes; w, amp: V arrays [leaves of the shape] f32; t: [T] f32 -> [V, T] f32, every add the tree's own.  Voices
    of equal shape are evaluated together, frames in slices of about `budget` leaf values."""
    t = np.ascontiguousarray(t, _F)
    out = np.empty((len(shapes), len(t)), _F)
    groups = {}
    for v, s in enumerate(shapes):
        groups.setdefault(plain(s), []).append(v)
    for s, vs in groups.items():
        P = n_leaves(s)
        wg = np.stack([np.asarray(w[v], _F) for v in vs])
        ag = np.stack([np.asarray(amp[v], _F) for v in vs])
        assert wg.shape == ag.shape == (len(vs), P), (s, wg.shape, ag.shape)
        tstep = max(1, budget // (P * len(vs)))
        for t0 in range(0, len(t), tstep):
            r, pos = _eval(s, bank_reference._leaves(wg, ag, t[t0:t0 + tstep]), 0)
            assert pos == P
            out[vs, t0:t0 + tstep] = r
    return out


def render_sum_tree(shapes, w, amp, t):
    """The same leaves in the synth.sum_tree association (what tests/bank_reference.py restates): the sensitivity yardstick."""
    t = np.ascontiguousarray(t, _F)
    return np.stack([bank_reference.render_bank(np.asarray(w[v], _F)[None], np.asarray(amp[v], _F)[None], t)[0] for v in range(len(shapes))])


# ---- the graph -------------------------------------------------------------------------------------------------------------------

def build_graph(shapes, w, amp, time_slot=0):
    """One graph, voice v of shape shapes[v] on output row v: synth.partial_leaves + synth.sum_tree for the integers,
    g.binop(K_SUM2, a, b) for the pairs.  Leaves that no node uses (the second operand of same(), a shared sub-tree after its
    first voice) are not made."""
    g = synth.GraphArrays()
    made = {}
    roots = []
    for v, shape in enumerate(shapes):
        wv, av = np.asarray(w[v], _F), np.asarray(amp[v], _F)
        assert wv.shape == av.shape == (n_leaves(shape),), (v, shape, wv.shape)
        need = np.zeros(len(wv), bool)
        seen = set(made)

        def mark(s, pos):
            if isinstance(s, int):
                need[pos:pos + (1 << s)] = True
            elif s[0] == "same":
                mark(s[1], pos)
            elif s[0] == "shared":
                if s[1] not in seen:
                    seen.add(s[1])
                    mark(s[2], pos)
            else:
                mark(s[0], pos)
                mark(s[1], pos + n_leaves(s[0]))

        mark(shape, 0)
        lv = np.zeros(len(wv), np.uint32)
        lv[need] = synth.partial_leaves(g, wv[need], av[need], time_slot)

        def node(s, pos):
            if isinstance(s, int):
                h = lv[pos:pos + (1 << s)]
                assert h.all()
                return int(synth.sum_tree(g, h[None])[0]) if s else int(h[0])
            if s[0] == "same":
                x = node(s[1], pos)
                return int(g.binop(synth.K_SUM2, np.array([x], np.uint32), np.array([x], np.uint32), 1)[0])
            if s[0] == "shared":
                if s[1] not in made:
                    made[s[1]] = node(s[2], pos)
                return made[s[1]]
            a = node(s[0], pos)
            b = node(s[1], pos + n_leaves(s[0]))
            return int(g.binop(synth.K_SUM2, np.array([a], np.uint32), np.array([b], np.uint32), 1)[0])

        roots.append(node(shape, 0))
    g.edge(np.array(roots, np.uint32), 0, 0, np.arange(len(roots), dtype=np.uint32))
    return g.finish(len(roots))


# ---- the table -------------------------------------------------------------------------------------------------------------------

def _positions(k):
    """Item k as the first, a middle and the last item of one voice: (k, (x, (k, (y, k)))) with x, y of other sizes."""
    x = 5 if k == 4 else 4
    y = 2 if k == 1 else 1
    return rchain([k, x, k, y, k])


_S = ((0, 1), 3)                                           # the sub-tree two voices share: 11 leaves


def _named():
    t = [(f"pos_k{k}", _positions(k)) for k in range(MAX_ITEM_LOG2 + 1)]
    t += [(f"pos_k{k}_left", lchain([k, 5 if k == 4 else 4, k, 2 if k == 1 else 1, k])) for k in (0, 1, 2, 3, 4, 5, 7)]
    t += [
        ("two_2048_and_a_leaf", (12, 0)),                                    # 2^12 complete leaves beside one leaf
        ("leaf_and_two_2048", (0, 12)),
        ("big_probe", ((11, (0, 11)), 4)),
        # chains of single leaves, pairs, 4s and 8s (a right chain's innermost pair of equal items is one item of twice the size)
        ("right_singles_12", rchain([0] * 12 + [2])),                        # (deeper right chains of singles: depth_15 .. depth_17)
        ("left_singles_20", lchain([0] * 20)),
        ("left_singles_40", lchain([0] * 40)),
        ("right_pairs_10", rchain([1] * 10)),
        ("left_pairs_10", lchain([1] * 10)),
        ("right_fours_7", rchain([2] * 7)),
        ("left_fours_7", lchain([2] * 7)),
        ("right_eights_6", rchain([3] * 6)),
        ("left_eights_6", lchain([3] * 6)),
        # stack depths: 14 / 15 / 16 single leaves above a pair
        ("depth_15", rchain([0] * 14 + [1])),
        ("depth_16", rchain([0] * 15 + [1])),
        ("depth_17", rchain([0] * 16 + [1])),                                 # the outer add becomes a program
        ("depth_16_big_last", rchain([0] * 15 + [6])),                        # 15 merges after a split item
        ("depth_16_mixed", rchain([0, 1, 2, 3, 4, 0, 1, 2, 3, 5, 0, 1, 2, 3, 0, 4])),
        ("depth_16_then_items", (rchain([0] * 15 + [1]), (5, (3, 0)))),       # the stack falls to one level and rises again
        # 15 and 16 leaves
        ("left_15", lchain([0] * 15)),                                        # no voice: a stage program
        ("right_15", rchain([0] * 13 + [1])),
        ("left_16", lchain([0] * 16)),
        ("sixteen_3_2_2", ((3, 2), (1, (0, 0)))),                             # = ((3, 2), 2)
        ("sixteen_pairs", lchain([1] * 8)),
        # hand-over buffers: three and more items of >= 32 leaves in a row, then with small items between them
        ("big_run_right", rchain([5, 6, 5, 7])),
        ("big_run_left", lchain([6, 5, 7, 5, 8])),
        ("big_run_5", rchain([5, 6, 5, 6, 5, 7, 5])),
        ("big_run_smalls_between", rchain([5, 0, 6, 2, 5, 4, 7])),
        ("big_run_smalls_between_left", lchain([6, 1, 5, 3, 7, 0, 5, 4, 6])),
        ("sixteens_and_smalls", rchain([4, 0, 4, 1, 4, 2, 4, 3])),
        ("squares", lchain([5, 0, 5, 5, 1, 6, 5])),
        # mirrored operand orders
        ("128_plus_3", (7, ((0, 0), 0))),
        ("3_plus_128", (((0, 0), 0), 7)),
        ("lopsided", ((4, (0, 2)), ((1, 0), 5))),
        ("lopsided_mirrored", mirror(((4, (0, 2)), ((1, 0), 5)))),
        # DAGs: both operands one node; two voices that share a sub-tree
        ("same_operands", same((4, 0))),
        ("same_operands_deep", (same((2, (1, 0))), same((4, same((0, 1)))))),
        ("shares_a", (4, shared("S", _S))),
        ("shares_b", (shared("S", _S), (2, 0))),
    ]
    return t


def _random_shape(rng, d):
    if d == 0 or rng.random() < 0.3:
        return int(rng.choice([0, 0, 1, 2, 3, 4, 5, 6]))
    return (_random_shape(rng, d - 1), _random_shape(rng, d - 1))


def _randoms(n=30):
    rng = np.random.default_rng(SEED)
    out = []
    while len(out) < n:
        s = _random_shape(rng, 6)
        if not isinstance(s, int) and MIN_LEAVES <= n_leaves(s) <= 300 and _complete(plain(s)) < 0 and served(s):
            out.append((f"random_{len(out)}", s))
    return out


TABLE = _named() + _randoms()
SHAPES = dict(TABLE)
assert len(SHAPES) == len(TABLE)
BIG_LEAVES = 4096                                         # voices of this many leaves and more: a case of their own, fewer frames


def names(max_leaves=None, min_leaves=0, only_served=False):
    return [n for n, s in TABLE if min_leaves <= n_leaves(s) and (max_leaves is None or n_leaves(s) <= max_leaves) and (not only_served or served(s))]


# ---- per-voice parameters --------------------------------------------------------------------------------------------------------

VARIANTS = ("regular", "zero_amp", "silent_neg", "silent_pos", "mixed", "all_neg", "one_pos_padded", "one_pos_16", "one_pos_big")
SILENT = ("silent_neg", "silent_pos")
ZERO_SIGN = {v: (-0.0 if v in ("silent_neg", "all_neg") else 0.0) for v in VARIANTS}   # the root at a frame of t = +0.0


def _item_of(shape, pick):
    """The last leaf of the first item whose k satisfies `pick`, or None."""
    sch = schedule_of(shape)
    for k, off in zip(sch["items"], sch["offsets"]):
        if pick(k):
            return off + (1 << k) - 1
    return None


def has_variant(shape, variant):
    if variant == "one_pos_padded":
        return _item_of(shape, lambda k: k < 3) is not None
    if variant == "one_pos_16":
        return _item_of(shape, lambda k: k == 4) is not None
    if variant == "one_pos_big":
        return _item_of(shape, lambda k: k >= 5) is not None
    return True


def _tie(s, w, amp, pos, store):
    """Gives the leaves that stand for one node the same parameters."""
    if isinstance(s, int):
        return pos + (1 << s)
    if s[0] == "same":
        n = n_leaves(s[1])
        _tie(s[1], w, amp, pos, store)
        w[pos + n:pos + 2 * n], amp[pos + n:pos + 2 * n] = w[pos:pos + n], amp[pos:pos + n]
        return pos + 2 * n
    if s[0] == "shared":
        n = n_leaves(s[2])
        if s[1] in store:
            w[pos:pos + n], amp[pos:pos + n] = store[s[1]]
        else:
            _tie(s[2], w, amp, pos, store)
            store[s[1]] = (w[pos:pos + n].copy(), amp[pos:pos + n].copy())
        return pos + n
    return _tie(s[1], w, amp, _tie(s[0], w, amp, pos, store), store)


def voice(shape, variant, seed, store=None):
    """(w, amp) [leaves] of one voice.  Regular: a fundamental of 55 Hz .. 220 Hz a quarter down, distinct partials, amp = 1 / (k + 1)
    -- as tests/test_hip_bank_matrix.py's voices.  The variants:
      zero_amp     one amplitude +0                           silent_neg / silent_pos   every amplitude -0 / +0
      mixed        +0, -0 and sounding amplitudes in turn     all_neg                   every amplitude negative
      one_pos_*    all_neg with ONE positive amplitude, on the last leaf of the voice's first padded item (fewer than 8 leaves),
                   first item of 16 leaves or first item of 32 leaves and more.
    On a frame of t = +0.0 every leaf is an exact zero with its amplitude's sign: all_neg and silent_neg give -0 there, every
    other variant +0 (ZERO_SIGN)."""
    P = n_leaves(shape)
    rng = np.random.default_rng([SEED, seed])
    k = np.arange(P)
    f0 = _F(55.0 * 2.0 ** (rng.integers(0, 24) / 12.0))
    w = ((f0 * (k + 1).astype(_F)) / _F(48000.0) * _F(0.25) + (rng.random(P) * 1e-3).astype(_F)).astype(_F)
    amp = (_F(1.0) / (k + 1).astype(_F)).astype(_F)
    if variant == "zero_amp":
        amp[P // 3] = 0.0
    elif variant == "silent_neg":
        amp[:] = -0.0
    elif variant == "silent_pos":
        amp[:] = 0.0
    elif variant == "mixed":
        amp = np.where(k % 5 == 0, _F(0.0), np.where(k % 5 == 1, _F(-0.0), amp)).astype(_F)
    elif variant == "all_neg" or variant.startswith("one_pos"):
        amp = -amp
        if variant != "all_neg":
            at = _item_of(shape, {"one_pos_padded": lambda q: q < 3, "one_pos_16": lambda q: q == 4, "one_pos_big": lambda q: q >= 5}[variant])
            assert at is not None, (shape, variant)
            amp[at] = -amp[at]
    else:
        assert variant == "regular", variant
    _tie(shape, w, amp, 0, {} if store is None else store)
    return w, amp


def voices(entries, seeds=None):
    """entries: [(shape name, variant)] -> (shapes, w, amp) of one graph, voice v seeded by v (or seeds[v]); shared sub-trees tied
    across it."""
    store = {}
    shapes = [SHAPES[n] for n, _ in entries]
    params = [voice(SHAPES[n], var, v if seeds is None else seeds[v], store) for v, (n, var) in enumerate(entries)]
    return shapes, [p[0] for p in params], [p[1] for p in params]


# the shapes that carry every variant: each has padded items, an item of 16 and items of >= 32 leaves
VARIANT_SHAPES = ("pos_k5", "pos_k7", "big_run_smalls_between", "big_run_smalls_between_left", "depth_16_mixed", "lopsided", "random_1", "random_14")


def table_entries(shape_names, silent=True, variants=True):
    """Every shape regular; with `silent` every shape again as silent_neg; with `variants` the VARIANT_SHAPES among them in
    every other variant they have."""
    e = [(n, "regular") for n in shape_names]
    if silent:
        e += [(n, "silent_neg") for n in shape_names]
    if variants:
        e += [(n, var) for n in shape_names if n in VARIANT_SHAPES for var in VARIANTS
              if var != "regular" and not (silent and var == "silent_neg") and has_variant(SHAPES[n], var)]
    return e


# ---- time rows -------------------------------------------------------------------------------------------------------------------

OFFSET = (1 << 20) + 37
HOSTILE_NEG = np.array([-1e-9, -1e-30, -1e-45, -1e-20, -0.3, -2.5, -1e-7, -0.75, -3e-39, -1.5e-8, -0.001, -17.25], np.float32)
HOSTILE_ODD = np.array([np.nan, np.inf, -np.inf, 1e30, 3e38, 4294967296.0, 8e9, -0.0, 1e-45, 3e-39, 0.625, 2.5e-7], np.float32)
ZERO_FRAMES = (3, 17, 40)                                 # t = +0.0 here: three exact-zero results in the first tile


def hostile_row(idx, T):
    """tests/test_hip_bank_matrix.py's two hostile waves (both also in a call of 70 frames) plus three frames of t = +0.0 in the
    first tile."""
    row = synth.time_ramp(idx, idx + T)
    a = max(0, min(64 + 5, T - len(HOSTILE_NEG) - len(HOSTILE_ODD) - 2))
    row[a:a + len(HOSTILE_NEG)] = HOSTILE_NEG
    b = T - len(HOSTILE_ODD) - 1
    if b >= a + len(HOSTILE_NEG):
        row[b:b + len(HOSTILE_ODD)] = HOSTILE_ODD
    for z in ZERO_FRAMES:
        if z < min(a, T):
            row[z] = 0.0
    return row


# ---- block streaming -------------------------------------------------------------------------------------------------------------

# Two patches of at most 32 schedule voices (one workgroup each) for bank_stream_general_kernel: the depth and chain shapes, and
# the item sizes and hand-over shapes up to about 3000 leaves; each with voices whose roots are exact zeros (the sign pass).
STREAM_PATCHES = {
    "depths_and_chains": [(n, "regular") for n in (
        "right_singles_12", "left_singles_20", "left_singles_40", "right_pairs_10", "left_pairs_10", "right_fours_7", "left_fours_7",
        "right_eights_6", "left_eights_6", "depth_15", "depth_16", "depth_16_big_last", "depth_16_mixed", "depth_16_then_items", "left_16",
        "sixteen_3_2_2", "sixteen_pairs", "128_plus_3", "3_plus_128", "lopsided", "lopsided_mirrored", "same_operands", "same_operands_deep",
        "shares_a", "shares_b")] + [("depth_16_mixed", "silent_neg"), ("left_singles_20", "silent_pos"), ("depth_16", "all_neg")],
    "items_and_hand_over": [(f"pos_k{k}", "regular") for k in range(11)] + [(n, "regular") for n in (
        "pos_k5_left", "pos_k7_left", "big_run_right", "big_run_left", "big_run_5", "big_run_smalls_between", "big_run_smalls_between_left",
        "sixteens_and_smalls", "squares", "random_0", "random_1", "random_2", "random_5", "random_9")] + [
        ("big_run_smalls_between", "silent_neg"), ("pos_k7", "silent_pos"), ("pos_k5", "one_pos_big"), ("pos_k1", "mixed")],
}


ZERO_RUN = tuple(range(5, 11))                            # t = +0.0 here: six exact-zero results in the first tile


def second_row(idx, T):
    """The row of the call of another length: the ramp with a run of six frames of t = +0.0 (more than 4 zero results in one
    tile: the zero-sign pass over all 64 frames, with either outcome by the voice's variant)."""
    row = synth.time_ramp(idx, idx + T)
    row[list(ZERO_RUN)] = 0.0
    return row


def sum_tree_shape(n):
    """The shape of synth.sum_tree over n leaves (adjacent pairs level by level, an odd one carried up)."""
    cur = [0] * n
    while len(cur) > 1:
        nxt = [(cur[i], cur[i + 1]) for i in range(0, len(cur) - 1, 2)]
        cur = nxt + cur[len(cur) - len(cur) % 2:] if len(cur) % 2 else nxt
    return cur[0]


def _leaf_pairs(s):
    return s if not isinstance(s, int) else 0 if s == 0 else (_leaf_pairs(s - 1), _leaf_pairs(s - 1))


def is_sum_tree(shape):
    """Whether the shape IS the sum_tree association of its leaves (the sensitivity yardstick cannot differ from it)."""
    def expand(s):
        return _leaf_pairs(s) if isinstance(s, int) else (expand(s[0]), expand(s[1]))
    return expand(plain(shape)) == sum_tree_shape(n_leaves(shape))
