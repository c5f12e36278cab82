"""Dense f32 reference for the staged graphs of tests/stage_variants.py (TEST INFRASTRUCTURE).

A graph is the raw form the engine's C ABI takes: {handle: primitive} and edges (from, to, from_slot, to_slot) -- handle 0
is the input side (from_slot = input slot) and the output side (to_slot = output row), an F32Constant's value rides in
from_slot.  `render` evaluates every node ONCE per frame over [0, end), forward in time, in numpy float32 with the
reference's operation order and rules (reference.rs:178-265, as oracle/ref_numpy.py restates them):
    Sum2 / Multiply / Divide   one IEEE f32 operation (a then b)
    Modulo                     fmodf, then + b when the result is negative
    Minimum                    (a < b || b != b) ? a : b; "sparkle": a NaN left operand wins
    Delay                      the amount, per frame, becomes frames: NaN or negative -> 0, >= 2^64 -> the output is 0, else
                               floor; "sparkle": an amount that is not >= 0 makes the output 0; before time 0 the value is 0
    input reads                out of range (beyond what the store holds) -> 0
The oracle recurses per sample without memoisation; every node is a pure function of the frame, so evaluating each (node,
frame) once gives the same bits.  Nodes outside feedback loops are evaluated over all frames at once.  A loop (a strongly
connected set of nodes) is evaluated in blocks of its smallest Delay: within a block no node reads a value of the same
block through a Delay of the loop, so each block is one vectorised pass in dependency order.

Input store (InputStore): per slot an array indexed by absolute frame, kept as reference.rs:47-86 keeps it for calls
that pass one full-length row per input slot -- a seek (a call not starting where the last one ended) forgets every
slot's history (zeros before the call), a contiguous call appends.  The cases avoid the store's other rules: every call
passes rows of the call's full length (no last-value padding of short rows), and the first call passes no more rows
than n_slots * n_times (the store's vector count: rows beyond it are dropped).
"""
import numpy as np

TWO64 = np.float32(18446744073709551616.0)
F0 = np.float32(0.0)


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


class Graph:
    """Nodes and edges in the C ABI's terms; `c(value)` makes an edge source from constant node 1."""

    def __init__(self):
        self.nodes = {1: "F32Constant"}
        self.edges = []
        self._next = 2

    def node(self, kind):
        h = self._next
        self._next += 1
        self.nodes[h] = kind
        return h

    def edge(self, frm, to, from_slot, to_slot):
        self.edges.append((frm, to, from_slot, to_slot))

    def op(self, kind, a, b):
        """A binary node of sources a and b: a handle, ("in", slot) or ("c", value)."""
        h = self.node(kind)
        for slot, s in enumerate((a, b)):
            self.connect(s, h, slot)
        return h

    def connect(self, s, to, to_slot):
        if isinstance(s, tuple) and s[0] == "in":
            self.edge(0, to, s[1], to_slot)
        elif isinstance(s, tuple) and s[0] == "c":
            self.edge(1, to, f32_bits(s[1]), to_slot)
        else:
            self.edge(s, to, 0, to_slot)

    def output(self, s, row):
        self.connect(s, 0, row)

    def install(self, r):
        for h, kind in self.nodes.items():
            r.on_add_node(h, kind)
        for e in self.edges:
            r.on_add_edge(*e)

    @property
    def n_out(self):
        return max(e[3] for e in self.edges if e[1] == 0) + 1


class InputStore:
    """reference.rs:47-86 for full-length rows: per slot, the values by absolute frame."""

    def __init__(self):
        self.rows = []
        self.head = 0
        self.dirty_from = 0      # the first frame whose stored input the last call changed (DenseReference resumes there)

    def call(self, idx, rows):
        n = len(rows[0]) if rows else 0
        assert all(len(r) == n for r in rows), "the cases pass full-length rows"
        self.dirty_from = idx
        if idx != self.head:
            self.rows = [np.zeros(idx, np.float32) for _ in self.rows]
            self.dirty_from = 0
        while len(self.rows) < len(rows):
            self.rows.append(np.zeros(idx, np.float32))
        for s, r in enumerate(rows):
            assert len(self.rows[s]) == idx
            self.rows[s] = np.concatenate([self.rows[s], np.asarray(r, np.float32)])
        for s in range(len(rows), len(self.rows)):     # (slots the call passes no row for: never the cases')
            self.rows[s] = np.concatenate([self.rows[s], np.zeros(n, np.float32)])
        self.head = idx + n


def _delay_frames(d, sparkle):
    """(live, frames) per frame for amounts d (reference.rs:200-215; ref_numpy.py's rule)."""
    with np.errstate(invalid="ignore"):
        live = ~(d >= TWO64)
        if sparkle:
            live &= d >= F0
        clamp = ~(d >= F0)
        dd = np.where(clamp | ~live, F0, d).astype(np.float64)
    hi = dd >= 2.0 ** 63
    frames = np.where(hi, dd - 2.0 ** 63, dd).astype(np.uint64) + np.where(hi, np.uint64(1) << np.uint64(63), np.uint64(0))
    return live, frames


def _sccs(succ, nodes):
    """Tarjan, iterative: the strongly connected components in reverse topological order of `succ` (node -> its sources)."""
    index, low, on, stack, out, counter = {}, {}, set(), [], [], [0]
    for root in nodes:
        if root in index:
            continue
        work = [(root, iter(succ[root]))]
        index[root] = low[root] = counter[0]
        counter[0] += 1
        stack.append(root)
        on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in index:
                    index[w] = low[w] = counter[0]
                    counter[0] += 1
                    stack.append(w)
                    on.add(w)
                    work.append((w, iter(succ[w])))
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == index[v]:
                    comp = []
                    while True:
                        w = stack.pop()
                        on.discard(w)
                        comp.append(w)
                        if w == v:
                            break
                    out.append(comp)
    return out


def render(g, inputs, idx, end, semantics="reference", start=0, prev=None):
    """The graph's output rows over [idx, end): float32 [n_out, end - idx].  `inputs`: per slot, values by absolute frame.
    `prev`: the node values of an earlier render (a dict, updated in place), valid on [0, start): only [start, end) is
    evaluated (inputs before `start` must be what they were)."""
    sparkle = semantics == "sparkle"
    inb = {h: {} for h in g.nodes}
    outs = {}
    for frm, to, fs, ts in g.edges:
        (outs if to == 0 else inb[to])[ts] = (frm, fs)
    val = prev if prev is not None else {}
    if start > min([len(v) for v in val.values()] + [end]):
        start = 0
    for h in list(val):
        keep = val[h][:start]
        val[h] = np.zeros(end, np.float32)
        val[h][:start] = keep

    def edge_at(e, t):
        """The value of edge e at frames t (uint64); None: no edge -> 0."""
        if e is None:
            return np.zeros(len(t), np.float32)
        frm, fs = e
        if frm == 0:
            row = inputs[fs] if fs < len(inputs) else np.zeros(0, np.float32)
            ok = t < len(row)
            return np.where(ok, row[np.where(ok, t, 0)] if len(row) else F0, F0).astype(np.float32)
        if g.nodes[frm] == "F32Constant":
            return np.full(len(t), np.uint32(fs).view(np.float32), np.float32)
        assert fs == 0
        return val[frm][t.astype(np.int64)]

    def eval_node(h, t):
        kind = g.nodes[h]
        e = inb[h]
        if h in cut:                                     # a loop's Delay: a constant amount, floor(d) >= 1 frames
            d = cut[h]
            out = np.zeros(len(t), np.float32)
            live = t >= np.uint64(d)
            if live.any():
                out[live] = edge_at(e.get(0), t[live] - np.uint64(d))
            return out
        if kind == "Delay":
            live, frames = _delay_frames(edge_at(e.get(1), t), sparkle)
            live &= t >= frames
            out = np.zeros(len(t), np.float32)
            if live.any():
                out[live] = edge_at(e.get(0), t[live] - frames[live])
            return out
        a, b = edge_at(e.get(0), t), edge_at(e.get(1), t)
        with np.errstate(all="ignore"):
            if kind == "Sum2":
                return a + b
            if kind == "Multiply":
                return a * b
            if kind == "Divide":
                return a / b
            if kind == "Minimum":
                r = np.where((a < b) | (b != b), a, b)
                return np.where(a != a, a, r) if sparkle else r
            if kind == "Modulo":
                rem = np.fmod(a, b)
                return np.where(rem < F0, rem + b, rem)
        raise AssertionError(kind)

    # dependencies: every inbound node edge (a Delay's source too: it is read at earlier frames of the same array)
    work = [h for h in g.nodes if g.nodes[h] != "F32Constant"]
    succ = {h: [s for s, _ in inb[h].values() if s != 0 and g.nodes[s] != "F32Constant"] for h in work}
    frames_all = np.arange(end, dtype=np.uint64)
    frames_new = frames_all[start:]
    cut = {}
    for comp in _sccs(succ, work):
        if len(comp) == 1 and comp[0] not in succ[comp[0]]:
            h = comp[0]
            if h not in val:
                val[h] = np.zeros(end, np.float32)
            val[h][start:] = eval_node(h, frames_new)
            continue
        members = set(comp)
        # a loop: every cycle runs through a Delay of constant amount >= 1 (the engine refuses the others, FR_ERR_CYCLE);
        # within a block of its smallest such Delay, the Delays of the loop read only earlier blocks
        cut.clear()
        for h in comp:
            if g.nodes[h] == "Delay" and inb[h].get(0, (0,))[0] in members:
                amt = inb[h].get(1)
                assert amt is not None and g.nodes.get(amt[0]) == "F32Constant", "a loop through a Delay of signal amount"
                d = np.uint32(amt[1]).view(np.float32)
                assert d >= 1 and d < TWO64, "a loop through a Delay of less than one frame"
                cut[h] = int(d)
        L = min(cut.values())
        # order within a block: the dependencies that are not loop Delays' sources
        inner = {h: [s for s in succ[h] if s in members and not (h in cut and inb[h][0][0] == s)] for h in comp}
        order = [c[0] for c in _sccs(inner, comp)]
        assert len(order) == len(comp), "a loop that no Delay breaks"
        for h in comp:
            if h not in val:
                val[h] = np.zeros(end, np.float32)
        for b0 in range(start, end, L):
            t = frames_all[b0:min(end, b0 + L)]
            for h in order:
                val[h][b0:b0 + len(t)] = eval_node(h, t)
        cut.clear()
    n_out = g.n_out
    t = np.arange(idx, end, dtype=np.uint64)
    return np.stack([edge_at(outs.get(r), t) for r in range(n_out)]).reshape(n_out, end - idx)


class DenseReference:
    """render() call after call: each call evaluates only from the first frame whose stored input changed."""

    def __init__(self, g, semantics="reference"):
        self.g, self.semantics, self.val = g, semantics, {}

    def __call__(self, store, idx, end):
        return render(self.g, store.rows, idx, end, self.semantics, start=store.dirty_from, prev=self.val)


def first_diff(got, exp, what):
    """'' when got == exp bit for bit (NaN == NaN, +0 != -0), else where and how they first differ."""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    if got.shape != exp.shape:
        return f"{what}: shape {got.shape} != {exp.shape}"
    gb, eb = got.view(np.uint32), exp.view(np.uint32)
    same = (gb == eb) | (np.isnan(got) & np.isnan(exp))
    if same.all():
        return ""
    bad = np.argwhere(~same)
    r, c = bad[0]
    return f"{what}: {len(bad)} samples differ, first at row {r} frame {c}: got {got[r, c]!r} ({gb[r, c]:#010x}), expected {exp[r, c]!r} ({eb[r, c]:#010x})"
