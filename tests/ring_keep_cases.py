"""Graphs, edit sequences and the expected launch arithmetic of FR_RING_KEEP (kept delay lines), shared by the simulator
tests (tests/test_ring_keep_sim.py) and the GPU tests (tests/test_hip_ring_keep.py).

The expected counts come from the structure of the graphs built here -- which voices have a chain, how many taps a chain
has, which delay each tap reads with -- never from running the engine.

The chain of a voice (effects patch, feed-forward):
    x0 = Multiply(C(gain_v), voice_v)                       a stage program, stored in a ring (tap 1 reads it delayed)
    xj = Sum2(x(j-1), Multiply(C(0.5^j), Delay(x(j-1), C(d_j))))   j = 1 .. TAPS, d_j = BASE * j
    row v = x_TAPS                                          read by nobody: no ring
so the rings of a voice are: the voice itself (filled by the bank kernel) and x0 .. x(TAPS-1) (one program each), and
the look-back of the voice's ring is d_1 + .. + d_TAPS frames."""
import numpy as np

from libfriendship_amd import synth
from libfriendship_amd.capi import f32_bits
from libfriendship_amd.synth import C, K_DELAY, K_MUL, K_SUM2

CONST = synth.CONST_HANDLE
OPT = {"FR_RING_KEEP": "1"}


from kat_replay import same_bits   # (bit-exact f32, NaN == NaN as elsewhere in the suite)


class Chains:
    """V voices x P partials, each behind a gain and a chain of feed-forward taps.  Remembers every handle an edit needs."""

    def __init__(self, V=6, P=64, taps=3, base=300.0, seed=0x5EED0031):
        self.V, self.P, self.taps, self.base = V, P, taps, float(base)
        self.g = synth.GraphArrays()
        self.p = synth.voice_params(V, P, seed, detune=True)
        self.leaves = synth.partial_leaves(self.g, self.p["w"], self.p["amp"]).reshape(V, P)
        self.roots = synth.sum_tree(self.g, self.leaves)
        self.gain = [np.float32(0.5 + 0.05 * v) for v in range(V)]
        self.x0 = self.g.binop(K_MUL, C(np.array(self.gain, np.float32)), self.roots, V)
        self.delays, self.sums = [], []
        x = self.x0
        for j in range(taps):
            dl = self.g.binop(K_DELAY, x, C(np.float32(self.base * (j + 1))), V)
            x = self.g.binop(K_SUM2, x, self.g.binop(K_MUL, C(np.float32(0.5 ** (j + 1))), dl, V), V)
            self.delays.append(dl)
            self.sums.append(x)
        self.g.edge(x, 0, 0, np.arange(V, dtype=np.uint32))
        self.tree = self.g.finish(V)
        self.next = int(self.g.next)
        self.rows = [int(h) for h in x]          # handle wired to output row v
        self.n_rows = V

    # ---- what the planner must come to -----------------------------------------------------------------------------
    def chain_rings(self):
        """Rings a voice's chain stores through programs: x0 .. x(taps-1)."""
        return self.taps

    def rings(self, voices=None):
        return (self.V if voices is None else voices) * (1 + self.chain_rings())

    def lookback(self, taps=None):
        """Frames the voice's own ring is read back: the sum of the chain's delays."""
        taps = self.taps if taps is None else taps
        return int(sum(self.base * (j + 1) for j in range(taps)))

    # ---- edits, each a function of a renderer ----------------------------------------------------------------------
    def edit_gain(self, v, value):
        old, new = self.gain[v], np.float32(value)

        def apply(r):
            r.on_del_edge(CONST, int(self.x0[v]), f32_bits(old), 0)
            r.on_add_edge(CONST, int(self.x0[v]), f32_bits(new), 0)
        self.gain[v] = new
        return apply

    def edit_amp(self, v, k, value):
        leaf = int(self.leaves[v, k])
        old, new = np.float32(self.p["amp"][v, k]), np.float32(value)

        def apply(r):
            r.on_del_edge(CONST, leaf, f32_bits(old), 0)
            r.on_add_edge(CONST, leaf, f32_bits(new), 0)
        self.p["amp"][v, k] = new
        return apply

    def edit_tap_delay(self, v, j, value):
        """Tap j + 1 of voice v reads its source `value` frames back instead of base * (j + 1)."""
        node = int(self.delays[j][v])
        old, new = np.float32(self.base * (j + 1)), np.float32(value)

        def apply(r):
            r.on_del_edge(CONST, node, f32_bits(old), 1)
            r.on_add_edge(CONST, node, f32_bits(new), 1)
        return apply

    def note_on(self, seed=0x5EED0077):
        """One more voice with its chain on one more output row.  Returns (apply, new row count)."""
        g = synth.GraphArrays()
        g.next = self.next
        g.handles, g.kinds = [], []
        p = synth.voice_params(1, self.P, seed, detune=True)
        p["w"] = (p["w"] * np.float32(1.37)).astype(np.float32)
        root = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(1, self.P))
        x = g.binop(K_MUL, C(np.float32(0.8)), root, 1)
        for j in range(self.taps):
            dl = g.binop(K_DELAY, x, C(np.float32(self.base * (j + 1))), 1)
            x = g.binop(K_SUM2, x, g.binop(K_MUL, C(np.float32(0.5 ** (j + 1))), dl, 1), 1)
        row = self.n_rows
        g.edge(x, 0, 0, row)
        tree = {"handles": np.concatenate(g.handles), "kinds": np.concatenate(g.kinds),
                "edges": np.ascontiguousarray(np.concatenate(g.edges, axis=0), dtype=np.uint32)}
        self.next = int(g.next)
        self.n_rows += 1
        self.rows.append(int(x[0]))
        return (lambda r: synth.install(r, tree)), self.n_rows

    def delete_voice_row(self, v):
        """Output row v is re-pointed at the last row's chain and the last row dropped: voice v's rings leave the plan, the
        rings behind it renumber.  Returns (apply, new row count)."""
        last = self.n_rows - 1
        hv, hl = self.rows[v], self.rows[last]

        def apply(r):
            r.on_del_edge(hv, 0, 0, v)
            r.on_del_edge(hl, 0, 0, last)
            r.on_add_edge(hl, 0, 0, v)
        self.rows[v] = hl
        self.rows.pop()
        self.n_rows -= 1
        return apply, self.n_rows


def comb_patch(V=4, P=8, d=100, g=0.6, tap=None, seed=0x5EED0041):
    """x_v = voice_v + g * Delay(x_v, d) around each of V bank voices; row v = Multiply(C(out_gain_v), x_v) -- a gain behind
    the loop, outside it.  `tap`: (v, frames) adds row V = x_v + 0.5 * Delay(x_v, frames), a tap behind loop v.
    Returns (tree, handles) with handles = {"x", "delay", "fb_gain", "out", "g", "out_gain"}."""
    ga = synth.GraphArrays()
    p = synth.voice_params(V, P, seed, detune=True)
    roots = synth.sum_tree(ga, synth.partial_leaves(ga, p["w"], p["amp"]).reshape(V, P))
    x = ga.nodes(K_SUM2, V)
    dl = ga.binop(K_DELAY, x, C(np.float32(d)), V)
    m = ga.binop(K_MUL, dl, C(np.float32(g)), V)
    ga.edge(roots, x, 0, 0)
    ga.edge(m, x, 0, 1)
    out_gain = [np.float32(0.9 - 0.1 * v) for v in range(V)]
    out = ga.binop(K_MUL, C(np.array(out_gain, np.float32)), x, V)
    ga.edge(out, 0, 0, np.arange(V, dtype=np.uint32))
    n_out = V
    if tap is not None:
        tv, frames = tap
        t = ga.binop(K_DELAY, x[tv:tv + 1], C(np.float32(frames)), 1)
        y = ga.binop(K_SUM2, x[tv:tv + 1], ga.binop(K_MUL, C(np.float32(0.5)), t, 1), 1)
        ga.edge(y, 0, 0, V)
        n_out = V + 1
    tree = ga.finish(n_out)
    return tree, {"x": x, "delay": dl, "fb_gain": m, "out": out, "g": np.float32(g), "out_gain": out_gain, "d": np.float32(d), "next": int(ga.next)}


def merged_loop():
    """The two-node loop: x = in0 + Delay(y, 2), y = 0.5 * Delay(x, 3), row 0 = 0.7 * x (a gain outside the loop), row 1 = y.
    Returns a function installing it and the handles of the outside gain / the loop gain."""
    def install(r):
        r.on_add_node(1, "F32Constant")
        for h, k in ((2, "Sum2"), (3, "Delay"), (4, "Multiply"), (5, "Delay"), (6, "Multiply")):
            r.on_add_node(h, k)
        r.on_add_edge(0, 2, 0, 0)
        r.on_add_edge(3, 2, 0, 1)                    # x = in0 + Delay(y, 2)
        r.on_add_edge(4, 3, 0, 0)
        r.on_add_edge(1, 3, f32_bits(2.0), 1)
        r.on_add_edge(5, 4, 0, 0)                    # y = Delay(x, 3) * 0.5
        r.on_add_edge(1, 4, f32_bits(0.5), 1)
        r.on_add_edge(2, 5, 0, 0)
        r.on_add_edge(1, 5, f32_bits(3.0), 1)
        r.on_add_edge(1, 6, f32_bits(0.7), 0)        # row 0 = 0.7 * x
        r.on_add_edge(2, 6, 0, 1)
        r.on_add_edge(6, 0, 0, 0)
        r.on_add_edge(4, 0, 0, 1)
    return install


def swap_const(node, slot, old, new):
    def apply(r):
        r.on_del_edge(CONST, int(node), f32_bits(np.float32(old)), slot)
        r.on_add_edge(CONST, int(node), f32_bits(np.float32(new)), slot)
    return apply


def launches(plan, form):
    return ([b for b in plan["bank_launches"] if b.get("form") == form], [s for s in plan["stage_launches"] if s["form"] == form])


class Trio:
    """One sequence rendered three ways: the oracle, the engine with the option off, the engine with it on."""

    def __init__(self, lib, oracle_lib, install, extra_options=None, **kw):
        from libfriendship_amd.capi import Renderer
        self.off = Renderer(lib, options=dict(extra_options or {}), **kw)
        self.on = Renderer(lib, options=dict(extra_options or {}, **OPT), **kw)
        self.ref = Renderer(oracle_lib) if oracle_lib is not None else None
        self.all = [r for r in (self.off, self.on, self.ref) if r is not None]
        for r in self.all:
            install(r)
        self.idx = 0

    def edit(self, apply):
        for r in self.all:
            apply(r)

    def call(self, n_rows, T, rows=None, idx=None, oracle=True):
        """Renders [idx, idx + T) on all three; returns (plan of option off, plan of option on)."""
        if idx is not None:
            self.idx = idx
        i = self.idx
        rows = [synth.time_ramp(i, i + T)] if rows is None else rows
        a = self.off.fill_buffer(n_rows, i, i + T, rows)
        b = self.on.fill_buffer(n_rows, i, i + T, rows)
        assert same_bits(a, b), f"option on differs from option off at {i} (+{T}): {np.flatnonzero(a.view(np.uint32) != b.view(np.uint32))[:8]}"
        if self.ref is not None and oracle:
            e = self.ref.fill_buffer(n_rows, i, i + T, rows)
            assert same_bits(b, e), f"differs from the oracle at {i} (+{T}): {np.flatnonzero(b.view(np.uint32) != e.view(np.uint32))[:8]}"
        self.idx = i + T
        return self.off.plan(), self.on.plan()

    def close(self):
        for r in self.all:
            r.close()


# ---- the sequences, run on whichever library the caller hands in (simulator or HIP) ---------------------------------------

def ring_capacity(lookback, longest_call, feedback=False):
    """Floats per ring the engine needs: the power of two (at least 1024) that holds the look-back plus the longest call
    (a feedback plan: plus a replay chunk of 16384 frames)."""
    need, cap = lookback + max(longest_call, 16384 if feedback else 0), 1024
    while cap < need:
        cap <<= 1
    return cap


def total(notes, key):
    return sum(n[key] for n in notes)


def run_chain_sequence(lib, oracle_lib, V=6, P=64, taps=3, base=300.0, extra_options=None):
    """Case 1 of the feature: an effects chain per voice, one edit at a time, each followed by two calls."""
    ch = Chains(V, P, taps, base)
    t = Trio(lib, oracle_lib, lambda r: synth.install(r, ch.tree), extra_options)
    try:
        n, lb, per_voice = V, ch.lookback(), 1 + ch.chain_rings()
        longest = 0
        for T in (700, 1000, 256):                       # rings of 4096 frames wrap during the test
            off, on = t.call(n, T)
            longest = max(longest, T)
        assert on["ring_keep"] is True and off["ring_keep"] is False and "ring_state" not in off
        assert on["rings"] == ch.rings() and on["max_lookback"] == lb, on
        st = on["ring_state"]
        assert st["kept"] == ch.rings() and st["rebuilt"] == 0 and st["inert"] == "", st
        assert launches(on, "repair") == ([], []) and off["stage_launches"] == on["stage_launches"]

        def after_edit(T, rebuilt, voices, programs, frames, kept, moved=0):
            off, on = t.call(n, T)
            st = on["ring_state"]
            assert (st["rebuilt"], st["kept"]) == (rebuilt, kept), st
            assert (st["moved"] > 0) == (moved > 0) and st["move_launches"] == (1 if moved else 0), st
            banks, progs = launches(on, "repair")
            assert total(banks, "voices") == voices and total(progs, "programs") == programs, (banks, progs)
            assert all(b["frames"] == frames for b in banks) and all(s["frames"] == frames for s in progs), (banks, progs)
            assert st["repair_from"] == (t.idx - T - frames if rebuilt else t.idx - T), st
            assert launches(on, "replay") == ([], [])
            # the option-off renderer re-renders the whole window of every voice and every program
            assert total(off["bank_launches"], "voices") == n and off["bank_launches"][0]["frames"] == min(t.idx - T, off["max_lookback"]) + T, off["bank_launches"]
            off2, on2 = t.call(n, 300)                   # ... and the call after is a steady call on both
            assert on2["ring_state"]["kept"] == on2["rings"] and on2["ring_state"]["rebuilt"] == 0, on2["ring_state"]
            assert on2["stage_launches"] == off2["stage_launches"] and launches(on2, "repair") == ([], [])
            return on

        # a gain behind voice 2's bank: its chain's rings, none of its voice
        t.edit(ch.edit_gain(2, 0.33))
        after_edit(500, rebuilt=taps, voices=0, programs=taps, frames=lb, kept=ch.rings() - taps)
        # one partial's amplitude in voice 4: the voice over its look-back, and its chain
        t.edit(ch.edit_amp(4, 5, 0.123))
        after_edit(500, rebuilt=per_voice, voices=1, programs=taps, frames=lb, kept=ch.rings() - per_voice)
        # a note-on: the new voice only
        apply, n = ch.note_on()
        t.edit(apply)
        after_edit(400, rebuilt=per_voice, voices=1, programs=taps, frames=lb, kept=ch.rings())
        # a voice deleted: rings renumber, nothing is rebuilt
        apply, n = ch.delete_voice_row(1)
        t.edit(apply)
        after_edit(400, rebuilt=0, voices=0, programs=0, frames=0, kept=ch.rings(), moved=1)
        # a tap longer than anything its source ring can hold: the voice, its x0 and the two programs above the tap
        cap = ring_capacity(lb, 1000)
        t.edit(ch.edit_tap_delay(3, 0, float(cap + 500)))
        lb3 = cap + 500 + ch.lookback() - int(base)
        on = after_edit(400, rebuilt=per_voice, voices=1, programs=taps, frames=min(lb3, t.idx), kept=ch.rings() - per_voice, moved=1)
        assert on["max_lookback"] == lb3, on
        # a call four times longer than any before: the capacity grows, every ring is kept and moved, nothing repaired
        cap = ring_capacity(lb3, 1000)
        T = 4000
        while ring_capacity(lb3, T) == cap:
            T += 1000
        off, on = t.call(n, T)
        st = on["ring_state"]
        assert st["kept"] == ch.rings() and st["rebuilt"] == 0 and st["moved"] == ch.rings() and st["move_launches"] == 1, st
        assert launches(on, "repair") == ([], [])
        off, on = t.call(n, 300)
        # a seek back: everything rebuilt, as with the option off
        off, on = t.call(n, 300, idx=1000)
        st = on["ring_state"]
        assert st["kept"] == 0 and st["rebuilt"] == ch.rings() and st["moved"] == 0, st
        t.call(n, 300)
    finally:
        t.close()


def run_comb_sequence(lib, oracle_lib, d, reach=40000, V=4, P=64, first=(300, 700, 1000), step=8000, after=(500, 300), extra_options=None):
    """Case 2: combs around bank voices, a tap behind loop 2 (250 frames), contiguous calls to frame >= reach, then the edits,
    each followed by calls of `after` frames.  With an oracle every call is compared three ways; `oracle_lib` None: option off
    against option on only (the oracle's recursion costs frame / d voice evaluations per frame: the long sequence, in which
    the rings of 32768 frames wrap, is beyond it)."""
    A, B = after
    tree, h = comb_patch(V, P, d, tap=(2, 250))
    n = V + 1
    t = Trio(lib, oracle_lib, lambda r: synth.install(r, tree), extra_options)

    def call(T):
        return t.call(n, T)
    try:
        for T in first:
            off, on = call(T)
        assert on["feedback"] and on["feedback_loops"] == V and on["ring_state"]["inert"] == "", on
        while t.idx < reach:
            off, on = call(step)
        assert launches(on, "replay") == ([], []) and [s for s in off["stage_launches"] if s["form"] == "replay"] == []
        # a gain behind loop 3, outside every loop: nothing is replayed (without the option: everything, from frame 0)
        t.edit(swap_const(h["out"][3], 0, h["out_gain"][3], 0.25))
        off, on = call(A)
        assert launches(on, "replay") == ([], []) and launches(on, "repair") == ([], []), on["stage_launches"]
        assert on["ring_state"]["rebuilt"] == 1 and on["ring_state"]["moved"] == 0, on["ring_state"]
        assert total([s for s in off["stage_launches"] if s["form"] == "replay"], "programs") > 0, off["stage_launches"]
        call(B)
        # loop 1's gain: loop 1's program and voice 1, from frame 0, and nothing else
        t.edit(swap_const(h["fb_gain"][1], 1, h["g"], 0.4))
        off, on = call(A)
        banks, progs = launches(on, "replay")
        chunks = -(-(t.idx - A) // 16384)
        assert len(banks) == chunks and all(b["voices"] == 1 for b in banks), banks
        assert len(progs) == chunks and all(s["programs"] == 1 for s in progs), progs
        assert total(banks, "frames") == t.idx - A and total(progs, "frames") == t.idx - A
        call(B)
        # loop 1's Delay re-pointed: the loop is cut again and replayed, never taken for the old one
        t.edit(swap_const(h["delay"][1], 1, h["d"], float(d) + 3.0))
        off, on = call(A)
        banks, progs = launches(on, "replay")
        assert len(progs) >= 1 and total(progs, "frames") == t.idx - A, progs
        assert all(s["programs"] == 1 for s in progs) and all(b["voices"] == 1 for b in banks), (banks, progs)
        call(B)
        # a re-plan with an unchanged graph (the same constant written again): nothing rebuilt
        built = on["plans_built"]
        t.edit(swap_const(h["out"][0], 0, h["out_gain"][0], h["out_gain"][0]))
        off, on = call(A)
        assert on["plans_built"] > built, on
        st = on["ring_state"]
        assert st["rebuilt"] == 0 and st["kept"] == on["rings"] and st["moved"] == 0, st
        assert launches(on, "replay") == ([], []) and launches(on, "repair") == ([], [])
        assert total([s for s in off["stage_launches"] if s["form"] == "replay"], "programs") > 0
    finally:
        t.close()


def run_merged_loop(lib, oracle_lib, extra_options=None):
    """The merged two-node loop: an edit of the gain outside it replays nothing; an edit inside replays the one program."""
    t = Trio(lib, oracle_lib, merged_loop(), extra_options)
    rng = np.random.default_rng(3)
    try:
        def call(T):
            return t.call(2, T, rows=[rng.normal(size=T).astype(np.float32)])
        for T in (40, 100, 260):
            call(T)
        t.edit(swap_const(6, 0, 0.7, 0.3))
        off, on = call(50)
        assert on["feedback"] and launches(on, "replay") == ([], []), on["stage_launches"]
        assert total([s for s in off["stage_launches"] if s["form"] == "replay"], "programs") > 0
        call(30)
        t.edit(swap_const(4, 1, 0.5, 0.25))
        off, on = call(50)
        assert total(launches(on, "replay")[1], "programs") >= 1
        call(30)
    finally:
        t.close()


def run_random_edits(lib, oracle_lib, seeds, extra_options=None, calls=5):
    """Case 3, feed-forward: random graphs with random edits between calls through the staged evaluator.  No seed may be
    passed over: the oracle's own refusal must be the engine's, with and without the option."""
    import randgraph
    from libfriendship_amd.capi import RenderError
    refused = 0
    for seed in seeds:
        rng = np.random.default_rng(9000 + seed)
        steps, n_out = randgraph.random_graph(500 + seed, n_nodes=int(rng.integers(6, 30)), n_inputs=2, n_outputs=3, signal_delays=False, composites=True)
        t = Trio(lib, oracle_lib, lambda r: randgraph.install_steps(r, steps), extra_options, mode="staged")
        try:
            for k in range(calls):
                T = int(rng.integers(20, 90))
                rows = [synth.time_ramp(t.idx, t.idx + T), (rng.normal(size=T) * 3).astype(np.float32)]
                try:
                    exp = t.ref.fill_buffer(n_out, t.idx, t.idx + T, rows)
                except RenderError as e:
                    for r in (t.off, t.on):
                        try:
                            r.fill_buffer(n_out, t.idx, t.idx + T, rows)
                            raise AssertionError(f"seed {seed}: the oracle refuses call {k}, the engine does not")
                        except RenderError as e2:
                            assert e2.status == e.status, (seed, k)
                    refused += 1
                    break
                a = t.off.fill_buffer(n_out, t.idx, t.idx + T, rows)
                b = t.on.fill_buffer(n_out, t.idx, t.idx + T, rows)
                assert same_bits(a, exp), f"seed {seed} call {k}: option off differs from the oracle"
                assert same_bits(b, exp), f"seed {seed} call {k}: option on differs from the oracle {t.on.plan()['ring_state']}"
                t.idx += T
                edits = randgraph.random_edits(rng, steps, int(rng.integers(1, 4)), signal_delays=False)
                t.edit(lambda r: randgraph.install_steps(r, edits))
        finally:
            t.close()
    return refused


def run_random_feedback_edits(lib, oracle_lib, seeds, extra_options=None, calls=5):
    """Case 3, feedback: the generator of test_feedback_graphs_edited_during_playback.  Returns (seeds run, passed over with
    the option off, passed over with it on); a seed is passed over only where the renderer refuses a call."""
    import randgraph
    from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, RenderError, Renderer
    done = 0
    skipped = {"off": {}, "on": {}}        # seed -> (call, status) of the refusal that ended it
    for seed in seeds:
        made = randgraph.random_feedback_graph(seed, n_frames=20, budget=2e4)
        if made is None:
            continue
        done += 1
        for which, options in (("off", {}), ("on", OPT)):
            steps = list(made[0])
            n_out = made[1]
            rng = np.random.default_rng(seed + 5)
            with Renderer(lib, options=dict(extra_options or {}, **options)) as hip, Renderer(oracle_lib) as ref:
                randgraph.install_steps(hip, steps)
                randgraph.install_steps(ref, steps)
                idx, k_done = 0, -1
                try:
                    for k in range(calls):
                        T = int(rng.integers(3, 7))
                        rows = [rng.normal(size=T).astype(np.float32), rng.integers(-2, 5, size=T).astype(np.float32)]
                        got = hip.fill_buffer(n_out, idx, idx + T, rows)
                        exp = ref.fill_buffer(n_out, idx, idx + T, rows)
                        assert same_bits(got, exp), f"seed {seed}, option {which}, call {k}"
                        idx += T
                        k_done = k
                        edits = randgraph.safe_feedback_edits(rng, steps, 2)
                        randgraph.install_steps(hip, edits)
                        randgraph.install_steps(ref, edits)
                except RenderError as e:
                    assert e.status == FR_ERR_UNSUPPORTED, (seed, which, e)
                    skipped[which][seed] = (k_done + 1, e.status)
    assert skipped["on"] == skipped["off"], (skipped["off"], skipped["on"])   # the same call of the same seed, the same status
    return done, len(skipped["off"]), len(skipped["on"])


class Taps:
    """V voices, row v = voice_v + 0.5 * Delay(voice_v, d): exactly one ring per voice (the voice's own, filled by the bank
    kernel), so the plan has V rings."""

    def __init__(self, V, P=64, d=37.0, seed=0x5EED0055):
        self.V, self.d = V, float(d)
        g = synth.GraphArrays()
        p = synth.voice_params(V, P, seed, detune=True, wrap=48)
        roots = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))
        dl = g.binop(K_DELAY, roots, C(np.float32(d)), V)
        y = g.binop(K_SUM2, roots, g.binop(K_MUL, C(np.float32(0.5)), dl, V), V)
        g.edge(y, 0, 0, np.arange(V, dtype=np.uint32))
        self.tree = g.finish(V)
        self.rows = [int(h) for h in y]

    def drop_first(self):
        """Row 0 is re-pointed at the last row's node and the last row dropped: voice 0's ring leaves, the others renumber."""
        last = len(self.rows) - 1
        h0, hl = self.rows[0], self.rows[last]

        def apply(r):
            r.on_del_edge(h0, 0, 0, 0)
            r.on_del_edge(hl, 0, 0, last)
            r.on_add_edge(hl, 0, 0, 0)
        self.rows[0] = hl
        self.rows.pop()
        return apply, len(self.rows)


# Where the move happens.  Rings are 1024 frames as long as every call is at most 1024 - 37 frames; the moved span is
# [max(valid_from, idx - 1024), idx).  Source and destination capacities are powers of two and the destination's is at least
# the source's, so every wrap point of the destination is one of the source too: a span can cross the wrap in the source
# only, in both, or in neither -- never in the destination only.  Each arrangement: (calls before the move, what it shows).
MOVE_ARRANGEMENTS = {
    "source_only": (333, 401, 397),                 # idx = 1131: [107, 1131) crosses 1024; the 4096 ring does not wrap there
    "both": (901, 977, 955, 873, 811),              # idx = 4517: [3493, 4517) crosses 4096, the wrap of both capacities
    "neither": (("seek", 5001), 131),               # idx = 5132, valid from 4964: 168 frames inside one segment, odd ends
    "three_segments": (987, 985, 983, 3),           # idx = 2958: [1934, 2958) has a head, a whole segment boundary and a tail
}


def run_moves(lib, oracle_lib, rings, arrangement, grow):
    """Case 4: ring_move_kernel (the simulator: its host loop) through the engine.  `rings` rings after the move; `grow`:
    a call of 3001 frames takes the capacity 1024 -> 4096; else voice 0 is dropped and every ring changes its row at 1024 ->
    1024.  The two calls after read every moved frame through the taps (d = 37, calls of 77 and 515 frames: the second one
    reaches back across everything the first did not).  The oracle takes the sizes it can afford."""
    V = rings if grow else rings + 1
    tp = Taps(V)
    t = Trio(lib, oracle_lib if V <= 65 else None, lambda r: synth.install(r, tp.tree))
    try:
        n = V
        for c in MOVE_ARRANGEMENTS[arrangement]:
            if isinstance(c, tuple):
                t.call(n, 64, idx=c[1])
            else:
                t.call(n, c)
        if grow:
            off, on = t.call(n, 3001)
        else:
            apply, n = tp.drop_first()
            t.edit(apply)
            off, on = t.call(n, 129)
        st = on["ring_state"]
        assert on["rings"] == rings and st["rebuilt"] == 0 and st["kept"] == rings and st["moved"] == rings and st["move_launches"] == 1, (st, on["rings"])
        assert launches(on, "repair") == ([], [])
        t.call(n, 77)
        t.call(n, 515)
    finally:
        t.close()
