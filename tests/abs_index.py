"""The absolute sample index at 2^24, 2^31, 2^32, 2^40 and 2^62: the case table (plain data and recipes, importable without a
GPU), shared by tests/test_abs_index.py (CPU tier) and tests/test_hip_abs_index.py (the kernels).

`idx`, the absolute frame of a call's first sample, is a uint64 in the ABI and reaches the kernels as idx, w0, ring_t0, head,
first or base, the generated stage programs as `u64 t`, and on the host it drives the windows, the history floor, the input
store and a stream's seek rule.  A comparison or a difference of two of these that is taken in 32 bits gives the right answer
for every frame below 2^32 (some below 2^31, float conversions below 2^24), which is where every other test of the suite stays.

THE SHIFT RULE.  Every dense reference of the suite indexes its arrays from frame 0, so none can render at 2^32.  It does not
have to: a seek forgets every input (zeros before the call's first frame), Delay is the only operation that looks at other
frames, and the only thing it learns from the absolute frame t is whether t - amount is below 0.  So if the sequence's seek
points are at or above the case's whole look-back (every constant amount and the bound of every signal amount, summed along
the deepest path), and every amount that is not so bounded is negative, NaN or >= 2^64 (then it reads +0 wherever the call
is), no read lands before frame 0 in either run, and the output depends on idx only through idx - seek point:
    expected(sequence moved to B) = dense reference(the same sequence at low frames, the LOW TWIN), on every sample.
An amount such as 2^32, 8e9 or 1e10 lies between the low twin's frames and the high run's and would read +0 in one and a
sample in the other: the amount rows hold none.  tests/test_abs_index.py proves the rule per case and base against the C++
oracle rendered at the high frames directly (its input store keeps a zero prefix: no array of idx floats).

ROWS ARE DATA.  rebase() moves every idx and nothing else.  A time row is never a ramp of the moved idx: at idx >= 2^32 the f32
ramp has no fraction left in t * w, every voice is an exact zero, and zeros would be compared with zeros.  Time rows are the
ramp from TIME0 + (frame - seek base) on: around frame 3000 an ADSR envelope is in its sustain (a ramp from 65436 on lies past
the envelope's end, 48000: all rows zero).  test_abs_index.py asserts that at least half of the expected samples of every row
are finite and non-zero.

THE LOW SEQUENCE, in frames relative to its base S0 (after rebase: relative to B):
    seek to -100; contiguous calls that cross 0 in the middle of a call and of a 64-frame group; a 1-frame call; a call of 130;
    a seek forward to +5003; a seek back across 0 to -40; and, kept only for B <= 2^40, a far seek forward to +2^33 + 69.
The far seek's low twin lies at FAR_LOW: its segment begins with a seek like every other, so the rule holds for it with its own
seek point.  S0 is 65536 for graphs of a few nodes (pull, stage programs); for patches with voices it is 2048, since the dense
reference holds every node's value from frame 0 to the sequence's end (1024 partials x 11 nodes x 70 000 frames would be 3 GB);
their look-back is asserted to fit below S0 - 100 from fr_plan_json like everyone's."""
import zlib

import numpy as np

import stage_reference as sr
import stage_variants as sv
import stream_cases as K
import stream_dyn_cases as D
import stream_loop_cases as L
import stream_matrix as X
import stream_reference as SR
from libfriendship_amd import synth

BASES = [1 << 24, 1 << 31, 1 << 32, 1 << 40, 1 << 62]
EVERY_CASE = [1 << 24, 1 << 32, 1 << 62]            # the bases of each case's own GPU test
PER_FAMILY = [1 << 31, 1 << 40]                     # the bases of one GPU test per family
S0 = 65536
S0_VOICES = 2048
SEEK, FORWARD, BACK = -100, 5003, -40
FAR = (1 << 33) + 69
FAR_MAX_BASE = 1 << 40
FAR_LOW = 5469                                      # where the far segment's low twin lies, relative to S0
TIME0 = 3100                                        # the time row's value at the base: sustain of synth.adsr_envelope
NONZERO_SHARE = 0.5
FB_MAX_REPLAY = 1 << 28                             # csrc/callplan.hpp


def rebase(calls, B, s0=S0):
    """The sequence `calls` = [(idx, T, rows)] written around s0, moved to B: every idx by B - s0, the rows untouched.  The far
    segment (at s0 + FAR_LOW and beyond; always the sequence's tail) goes to B + FAR, and is left out above FAR_MAX_BASE."""
    out = []
    for idx, T, rows in calls:
        off = idx - s0
        if off >= FAR_LOW:
            if B > FAR_MAX_BASE:
                break
            off += FAR - FAR_LOW
        assert 0 <= B + off and B + off + T < 1 << 64
        out.append((B + off, T, rows))
    return out


def call_starts(T, first=64, head=(), again=False):
    """[(offset, frames)] of the low sequence for an entry point that takes calls of any length; T: the case's steady length
    (it crosses 0 at its 36th frame: mid-call, mid-group).  first: the first call's length (a track matrix needs n_rows * first
    input vectors); head: further contiguous calls between the first and the steady one; again: a second steady call behind
    the call of 130 (a call longer than the rings were sized for grows them and renders its window anew, level by level:
    the second one then runs the case's own form)."""
    at = SEEK + first
    out = [(SEEK, first)]
    for n in head:
        out.append((at, n))
        at += n
    out += [(at, T), (at + T, 1), (at + T + 1, 130)] + ([(at + T + 131, T)] if again else [])
    assert any(o < 0 < o + n - 1 and o % 64 for o, n in out) and out[-1][0] + out[-1][1] < FORWARD
    return out + [(FORWARD, 200), (BACK, 150), (FAR_LOW, 100), (FAR_LOW + 100, 64)]


STREAM_SEGMENTS = [(SEEK, 400), (FORWARD, 200), (BACK, 150), (FAR_LOW, 130)]   # blocks of stream_cases.FIRST_LENGTHS: 64, 64 (crosses 0), 1, 37 ...


def time_row(off, T):
    return synth.time_ramp(TIME0 + off, TIME0 + off + T)


def special_frames(calls, B, delays):
    """The frames of a rebased sequence at which the oracle is sought at the high index: the first and last of each call, B - 1, B,
    B + 1 and B + d for the case's delays -- as (call number, column)."""
    want = {B - 1, B, B + 1} | {B + d for d in delays}
    out = []
    for k, (idx, T, _) in enumerate(calls):
        cols = {0, T - 1} | {t - idx for t in want if idx <= t < idx + T}
        out += [(k, c) for c in sorted(cols)]
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------
# A case: name, family, kind ("calls": fr_fill_buffer / fr_fill_buffer_dense; "stream": fr_stream_block_rows; "mixed": a `script`
# of calls, streams and an edit over the sequence, see run_mixed), s0, `install(r)` (and `setup(r)`: fr_set_track_inputs),
# n_rows, semantics, options, mode, entry, `low()` -> the low sequence [(idx, T, rows)], `expected(low)` -> [float32 [n_rows, T]] by
# the dense reference, `delays` (constant amounts whose reads are sought at B + d), `deep` (some reader looks back more than 100
# frames: asserted from the plan), `check(plan, k, T)`: the kernel / key assertions after call k on the device; `edits`
# (optional): {call number: apply(renderer)}, graph edits made before that call.

def _stage_rows(case, n, rng, hostile):
    rows = [(rng.normal(size=n) * 3).astype(np.float32) for _ in range(case["n_in"])]
    if case["graph"][0] == "dyn_delays":   # whole and fractional frames below 64, some negative; hostile: NaN, -0, 2^64, +-inf ...
        for s, amounts in ((1, sv.HOSTILE_AMOUNTS), (2, sv.BOUNDED_AMOUNTS)):
            rows[s] = (rng.integers(-8, 60, size=n) + rng.integers(0, 4, size=n) * 0.25).astype(np.float32)
            if hostile:
                rows[s][1::3] = np.resize(amounts, len(rows[s][1::3]))
    if hostile:
        s = 0 if case["graph"][0] == "dyn_delays" else case["hostile"]
        rows[s][::5] = np.resize(sv.HOSTILE, len(rows[s][::5]))
    return rows


def _graph_expected(g, semantics):
    def expected(low):
        store, ref = sr.InputStore(), sr.DenseReference(g, semantics)
        out = []
        for idx, T, rows in low:
            store.call(idx, rows)
            out.append(ref(store, idx, idx + T))
        return out
    return expected


STAGE_LOOKBACK = {"chain": lambda a: sum(a[0]), "delayed_reads": lambda a: a[0], "many_inputs": lambda a: 1, "dyn_delays": lambda a: 2 + 64}


def _stage_case(c):
    g = sv.build(c)
    name, args = c["graph"]

    def low():
        rng = np.random.default_rng(zlib.crc32(c["key"].encode()))
        return [(S0 + off, n, _stage_rows(c, n, rng, hostile=(n == 130))) for off, n in call_starts(c["T"], again=True)]

    def check(plan, k, T):
        variants = [l["variant"] for l in plan["stage_launches"]]
        kern = sv.key_base(c["key"]).split("/")[0]
        assert plan["pull_rows"] == 0 and variants and not plan["feedback"], plan
        for v in variants:
            assert sv.unreachable(v, False, int(c["options"].get("FR_STAGE_BLOCK", 0)), plan["fused_carry_only"]) is None, (c["key"], v)
            assert v.split("/")[0] == kern, f"call {k}: ran {variants}, expected kernel {kern}"
        if T == c["T"] and (k == 4 or T <= 600):      # (k == 1, the call across B, unless it had to grow the rings; k == 4, the second steady call)
            assert sv.key_base(c["key"]) in variants, f"the steady call {k} ran {variants}, expected {c['key']}"

    delays = sorted(set(args[0])) if name == "chain" else [1, 2] if name != "delayed_reads" else [1, args[0]]
    return {"name": "stage:" + c["key"], "family": "compiled stage" if c["key"].startswith("jit_stage") else "stage interpreter", "kind": "calls",
            "s0": S0, "install": g.install, "n_rows": g.n_out, "semantics": c["semantics"], "options": c["options"], "mode": "auto",
            "entry": c["entry"], "low": low, "expected": _graph_expected(g, c["semantics"]), "delays": delays,
            "lookback": STAGE_LOOKBACK[name](args) if name == "chain" else None, "deep": STAGE_LOOKBACK[name](args) > 100, "check": check, "jit": c["key"].startswith("jit_stage"), "n_in": c["n_in"]}


def step_graph():
    """y = Delay(3.5, 150) * min(in0, in1) + Delay(min(in0, in1), 70): a Delay of a constant by a constant, which the planner makes
    an S_STEP (0 before frame 150, the constant from there on) -- no case of stage_variants has one.  Row 1: the step alone plus in0."""
    g = sr.Graph()
    x = g.op("Minimum", ("in", 0), ("in", 1))
    st = g.op("Delay", ("c", 3.5), ("c", 150.0))
    g.output(g.op("Sum2", g.op("Multiply", st, x), g.op("Delay", x, ("c", 70.0))), 0)
    g.output(g.op("Sum2", st, ("in", 0)), 1)
    return g


def _step_case(tag, options, kernel):
    g = step_graph()
    base = {"graph": ("step", ()), "n_in": 2, "hostile": 0}

    def low():
        rng = np.random.default_rng(zlib.crc32(tag.encode()))
        return [(S0 + off, n, _stage_rows(base, n, rng, hostile=(n == 130))) for off, n in call_starts(300)]

    def check(plan, k, T):
        variants = [l["variant"] for l in plan["stage_launches"]]
        assert plan["pull_rows"] == 0 and variants and all(v.startswith(kernel) for v in variants), (k, variants, plan["pull_rows"])

    return _case("stage:step/" + tag, "compiled stage" if kernel.startswith("jit") else "stage interpreter", S0, g.install, 2, options, low,
                 _graph_expected(g, "reference"), [70, 150], False, check, 2, jit=kernel.startswith("jit"))


def pull_graph():
    """A random graph of primitives with Delays of up to 300 frames, of constant and of signal amounts (tests/randgraph.py), as
    a stage_reference.Graph; three rows.  Seed 57 -- chosen on the reference alone, never by what an engine returns: the first
    seed whose three rows are each at least 90 % finite and non-zero there, each follow an input row (seed 9, the first to
    meet the share, renders three constants: a truncated input read could not show), and that has Delays by signal amounts
    beside constant ones above 100 frames.  Its Delays: 46 and 220 frames, and three by an input's or a node's value.  The CPU
    tier asserts the share and the dependence, and the oracle proves the shift rule for it."""
    import randgraph
    from libfriendship_amd.capi import PRIMITIVES
    steps, n_out = randgraph.random_graph(PULL_SEED, n_nodes=30, n_inputs=2, n_outputs=3, signal_delays=True, composites=False, max_delay=300)
    g = sr.Graph()
    g.nodes, g.edges = {}, []
    for s in steps:
        if s[0] == "node":
            g.nodes[s[1]] = PRIMITIVES[s[2].kind]
        else:
            g.edges.append(tuple(int(x) for x in s[1:]))
    return g


PULL_SEED = 57


def _pull_case():
    g = pull_graph()

    def low():
        rng = np.random.default_rng(77)
        out = []
        for off, n in call_starts(97):
            amounts = (rng.integers(-8, 260, size=n) + rng.integers(0, 4, size=n) * 0.25).astype(np.float32)
            if n == 130:
                amounts[1::3] = np.resize(sv.HOSTILE_AMOUNTS, len(amounts[1::3]))
            out.append((S0 + off, n, [(rng.normal(size=n) * 3).astype(np.float32), amounts]))
        return out

    def check(plan, k, T):
        assert plan["pull_rows"] == g.n_out and not plan["stage_launches"] and not plan["bank_launches"], plan

    return {"name": "pull:randgraph", "family": "pull", "kind": "calls", "s0": S0, "install": g.install, "n_rows": g.n_out, "semantics": "reference",
            "options": {}, "mode": "pull", "entry": "host", "low": low, "expected": _graph_expected(g, "reference"), "delays": [46, 220],
            "lookback": None, "deep": True, "check": check, "jit": False, "n_in": 2}


def _voice_expected(tree, semantics):
    return lambda low: SR.expected_blocks(tree, low, semantics)


BANK_TAPS = (150, 300, 450)                          # synth.effects_tree(taps=3, base_delay=150.0): look-back 900


def _bank_case(tag, T, options, kernel, V=4, P=128):
    """Voices into rings that a stage program reads 150, 300 and 450 frames back: the bank kernels' time_skip, time_valid and
    ring_t0 are live (the window starts before the call: before B, and before the seek point).  bank_short_kernel takes voices
    of at least 512 partials only (csrc/bankplan.hpp: log2_p >= 9), whatever the call's length: its case has two of those."""
    tree = synth.effects_tree(V, P, taps=3, base_delay=150.0)

    def low():
        return [(S0_VOICES + off, n, [time_row(off, n)]) for off, n in call_starts(T)]

    def check(plan, k, n):
        assert plan["pull_rows"] == 0 and plan["bank_launches"], plan
        if n == T:
            kernels = [b["kernel"] for b in plan["bank_launches"]]
            assert all(x.startswith(kernel) for x in kernels), f"the steady call ran {kernels}, expected {kernel}"

    return {"name": "bank:" + tag, "family": "bank to rings", "kind": "calls", "s0": S0_VOICES, "install": lambda r: synth.install(r, tree), "n_rows": V,
            "semantics": "reference", "options": options, "mode": "auto", "entry": "host", "low": low, "expected": _voice_expected(tree, "reference"),
            "delays": list(BANK_TAPS), "lookback": sum(BANK_TAPS), "deep": True, "check": check, "jit": kernel.startswith("jit"), "n_in": 1}


def _stream_low(c):
    """The blocks of stream_matrix.streams_of's recipes (time rows of stream_cases.finite_block_rows, control rows of
    stream_loop_cases.blocks_of through finite_controls, knob amounts), with the time rows' ramp from TIME0 on."""
    rng_t, rng = np.random.default_rng(c["time_seed"]), np.random.default_rng(zlib.crc32(c["name"].encode()))
    rows = K.finite_block_rows(rng_t, [(TIME0 + off, n) for off, n in STREAM_SEGMENTS])
    blocks = X.finite_controls(L.blocks_of([(idx - TIME0 + S0_VOICES, row) for idx, row in rows], rng, c["n_in"]))
    return D.knob_blocks(blocks) if c["knob"] else blocks


def _stream_case(c, family="stream", kernel_name=None):
    tree = c["build"]()
    kernel_name = kernel_name or X.KERNEL_NAME[c["kernel"]]
    delays = sorted({int(d) for d in SR.constant_delays(tree)})

    def check(plan, k, T):
        st = plan["stream"]
        assert st["servable"] and st["kernel"] == kernel_name, (c["name"], st)

    return {"name": "stream:" + c["name"], "family": family, "kind": "stream", "s0": S0_VOICES, "install": lambda r: synth.install(r, tree),
            "n_rows": c["n_rows"], "semantics": c["semantics"], "options": c["options"], "mode": "auto", "entry": "stream",
            "low": lambda: _stream_low(c), "expected": _voice_expected(tree, c["semantics"]), "delays": delays, "lookback": None,
            "deep": bool(delays) and sum(delays) > 100, "check": check, "jit": False, "n_in": c["n_in"]}


# ---- further call cases: observed bounds, kept rings, tracks ------------------------------------------------------------------

def _case(name, family, s0, install, n_rows, options, low, expected, delays, deep, check, n_in, kind="calls", entry="host", lookback=None, **more):
    return dict({"name": name, "family": family, "kind": kind, "s0": s0, "install": install, "n_rows": n_rows, "semantics": "reference", "options": options,
                 "mode": "auto", "entry": entry, "low": low, "expected": expected, "delays": list(delays), "lookback": lookback, "deep": deep,
                 "check": check, "jit": False, "n_in": n_in}, **more)


def _observed_case():
    """FR_DELAY_OBSERVED: y = x + 0.5 * Delay(x, 100 + 300 * In(1)), the bound taken from the rows seen (observed_delay_cases)."""
    import observed_delay_cases as O
    tree = O.delayed_voices(2, 128, "affine")

    def low():
        return [(S0_VOICES + off, n, [time_row(off, n), O.control_row(TIME0 + off, TIME0 + off + n, 0.0, 1.0)]) for off, n in call_starts(300)]

    def check(plan, k, T):
        assert plan["pull_rows"] == 0 and plan["bank_launches"] and plan["stage_launches"] and plan["max_lookback"] >= 400, plan

    return _case("observed:affine", "bank to rings", S0_VOICES, lambda r: synth.install(r, tree), 2, {"FR_DELAY_OBSERVED": "1"}, low,
                 _voice_expected(tree, "reference"), [100, 250, 400], True, check, 2)


class GraphRecorder:
    """The GraphWatcher calls of a renderer, kept as a stage_reference.Graph: what a sequence of edits leaves."""

    def __init__(self):
        self.nodes, self.edges = {}, []

    def on_add_nodes(self, handles, effect):
        from libfriendship_amd.capi import PRIMITIVES
        for h in handles:
            self.nodes[int(h)] = PRIMITIVES[effect.kind]

    def on_add_edges(self, edges):
        self.edges += [tuple(int(x) for x in e) for e in np.asarray(edges).reshape(-1, 4)]

    def on_add_edge(self, *e):
        self.edges.append(tuple(int(x) for x in e))

    def on_del_edge(self, *e):
        self.edges.remove(tuple(int(x) for x in e))

    def graph(self):
        g = sr.Graph()
        g.nodes, g.edges = dict(self.nodes), list(self.edges)
        return g


def _edited_expected(low, before, after, edit_at):
    """The dense reference of a sequence with one time row whose graph is `before` up to call edit_at and `after` from it on: per
    segment and graph, one render from the segment's first frame (a render is a pure function of graph and inputs)."""
    out = [None] * len(low)
    for seg in SR.segments_of(low):
        first = low[seg[0]][0]
        for g, ks in ((before, [k for k in seg if k < edit_at]), (after, [k for k in seg if k >= edit_at])):
            if not ks:
                continue
            end = low[ks[-1]][0] + low[ks[-1]][1]
            t = np.concatenate([np.zeros(first, np.float32)] + [low[k][2][0] for k in seg if low[k][0] < end])
            full = sr.render(g, [t], first, end)
            for k in ks:
                out[k] = full[:, low[k][0] - first:low[k][0] - first + low[k][1]].copy()
    return out


def _ring_keep_case():
    """FR_RING_KEEP (ring_keep_cases.Chains: voices behind a gain and taps of 150, 300 and 450 frames): between the two calls that
    straddle B, output row 1 is re-pointed at the last voice's chain and a new voice takes the last row -- the rings behind
    the deleted voice renumber (ring_move_kernel copies them: first, count), the new voice's are rebuilt over their look-back."""
    import ring_keep_cases as RK
    ch = RK.Chains(V=3, P=64, taps=3, base=150.0)
    drop, _ = ch.delete_voice_row(1)
    add, n_rows = ch.note_on()
    assert n_rows == 3

    def edit(r):
        drop(r)
        add(r)

    rec = GraphRecorder()
    synth.install(rec, ch.tree)
    before = rec.graph()
    edit(rec)
    after = rec.graph()

    def low():
        return [(S0_VOICES + off, n, [time_row(off, n)]) for off, n in call_starts(300)]

    def check(plan, k, T):
        assert plan["ring_keep"] is True and plan["pull_rows"] == 0 and plan["max_lookback"] == 900, plan
        if k == 1:
            st = plan["ring_state"]
            assert st["moved"] > 0 and st["move_launches"] == 1 and st["rebuilt"] == 4 and st["inert"] == "", st

    return _case("ring_keep:chains", "bank to rings", S0_VOICES, lambda r: synth.install(r, ch.tree), 3, {"FR_RING_KEEP": "1"}, low, lambda low: _edited_expected(low, before, after, 1),
                 [150, 300, 450], True, check, 1, lookback=900, edits={1: edit})


TRACK_V, TRACK_P = 3, 32


def _track_rows(off, n, rng):
    """A call's rows of synth.track_tree(TRACK_V, TRACK_P): the time row, then per partial a w row and an amp row, random per element
    (track_rows.regular_rows' recipe; w three times larger, as track_rows.span_rows has it for small frame numbers)."""
    k = TRACK_V * TRACK_P
    w = rng.random((k, n), dtype=np.float32) * np.float32(0.15)
    amp = (rng.random((k, n), dtype=np.float32) + np.float32(0.5)) * np.tile(np.float32(1.0) / np.arange(1, TRACK_P + 1, dtype=np.float32), TRACK_V)[:, None]
    rows = [time_row(off, n)]
    for i in range(k):
        rows += [w[i], amp[i]]
    return rows


def _track_case(name, tree, options, starts, delays, check, **more):
    def low():
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        return [(S0_VOICES + off, n, _track_rows(off, n, rng)) for off, n in starts]

    assert TRACK_V * starts[0][1] >= tree["n_inputs"]                 # the store keeps n_slots * n_times vectors: every row is live
    return _case(name, "tracks", S0_VOICES, lambda r: synth.install(r, tree), TRACK_V, options, low, _voice_expected(tree, "reference"), delays,
                 bool(delays), check, tree["n_inputs"], entry="dense", setup=lambda r: r.set_track_inputs(1), **more)


def _track_cases():
    import track_rows as TR

    def dense_check(plan, k, T):
        assert plan["pull_rows"] == 0 and [b["kernel"] for b in plan["bank_launches"]] == ["jit_bank"], plan["bank_launches"]

    def history_check(plan, k, T):
        # call 2 is longer than the delay rings hold: they are grown and lost, and the voices' window [B - 120, B + 1030) is
        # rendered from the track history in spans cut where its ring of 4096 frames wraps -- at B, a multiple of 4096 --, then the call
        n = len(plan["bank_launches"])
        assert plan["pull_rows"] == 0 and n == (3 if k == 2 else n) and n >= 1, (k, plan["bank_launches"])

    steady = call_starts(300, first=70)
    grown = call_starts(1000, first=70, head=(60,))
    assert grown[2] == (30, 1000)
    return [_track_case("tracks:dense", synth.track_tree(TRACK_V, TRACK_P), {}, steady, [], dense_check, setup_needs_jit=True),
            _track_case("tracks:history", TR.span_tree(TRACK_V, TRACK_P, 150), {"FR_TRACK_HISTORY": "4096"}, grown, [150], history_check)]


# ---- further stream cases: one of each later module --------------------------------------------------------------------------

def _module_stream_case(module, name, kernel, deep=None):
    """A case of stream_hist_cases / stream_taps_cases / stream_fx_cases, with stream_hist_cases.streams_of's rows."""
    import stream_hist_cases as H
    c = module.case(name)
    assert not c["knob"]

    def low():
        rng_t, rng = np.random.default_rng(0x415), np.random.default_rng(zlib.crc32(name.encode()))
        rows = K.finite_block_rows(H._FullBlocks(rng_t), [(TIME0 + off, n) for off, n in STREAM_SEGMENTS])
        return X.finite_controls(L.blocks_of([(idx - TIME0 + S0_VOICES, row) for idx, row in rows], rng, c["n_in"]))

    out = _stream_case(dict(c, kernel=None, name=name), kernel_name=kernel)
    out["low"] = low
    if deep is not None:
        out["deep"] = deep                                          # (fir: three reads of an input row, the deepest 100 frames back)
    return out


def _leaves_case():
    import stream_leaves_cases as LV
    c = LV.case("tri_128")
    d = {"name": c.name, "build": c.build, "n_rows": 2, "semantics": "reference", "options": c.options, "n_in": c.n_in, "oracle_frames": 0, "kernel": None}
    out = _stream_case(d, kernel_name=LV.KERNEL)
    out["low"] = lambda: [(idx - TIME0 + S0_VOICES, T, rows) for idx, T, rows in LV.blocks_of(c, [(TIME0 + off, n) for off, n in STREAM_SEGMENTS])]
    return out


def _more_stream_cases():
    import stream_fx_cases as FX
    import stream_hist_cases as H
    import stream_taps_cases as TP
    return [_module_stream_case(H, "eight_slots", H.NEW_KERNEL), _module_stream_case(TP, "env_taps_2x512", TP.case("env_taps_2x512")["kernel"]),
            _module_stream_case(FX, "fir", FX.NEW_KERNEL, deep=False), _leaves_case()]


# ---- a stream that stores what it is fed (FR_STREAM_STORE): fr_fill_buffer, an edit and streams mixed across B ---------------------
STORE_SCRIPT = [("fill", 0), ("begin",), ("block", 1), ("block", 2), ("block", 3), ("end",), ("edit",), ("begin",), ("block", 4), ("block", 5), ("block", 6),
                ("end",), ("fill", 7), ("begin",), ("block", 8), ("block", 9), ("end",), ("fill", 10), ("begin",), ("block", 11), ("block", 12), ("end",)]
STORE_STARTS = [(SEEK, 64), (SEEK + 64, 64), (28, 1), (29, 37), (66, 64), (130, 2), (132, 63), (195, 150),      # one segment: call, stream, edit, stream, call
                (FORWARD, 64), (FORWARD + 64, 37), (BACK, 150), (FAR_LOW, 64), (FAR_LOW + 64, 64)]


def _store_case():
    """stream_store_cases.tap_patch with a tap of 150 frames: fr_fill_buffer from B - 100, a stream that continues it across B
    (with the option a continuation, not a seek: its tap reads frames that fr_fill_buffer stored), a gain edited between two
    streams, fr_fill_buffer continuing the second; then a streamed seek forward, a seek back by fr_fill_buffer, the far seek streamed."""
    import stream_store_cases as ST
    p = ST.tap_patch(2, 128, ST.STORE, "tap_150", d=150.0)
    rec = GraphRecorder()
    p.install(rec)
    before = rec.graph()
    p.edits["gain"](rec)
    after = rec.graph()
    edit_at = 4

    def low():
        return [(S0_VOICES + off, n, [time_row(off, n)]) for off, n in STORE_STARTS]

    def check(plan, k, T):
        st = plan["stream"]
        assert st["servable"] and st["kernel"] == ST.NEW_KERNEL and st["store"]["on"] is True, st
        if k in (1, 4):
            assert st["store"]["continued"] is True, (k, st["store"])          # across B, and across the edit: no seek

    return _case("stream:store_tap_150", "stream", S0_VOICES, p.install, 2, dict(ST.STORE), low, lambda low: _edited_expected(low, before, after, edit_at),
                 [150], True, check, 1, kind="mixed", script=STORE_SCRIPT, edits={edit_at: p.edits["gain"]})


# ---- a streamed track voice (FR_STREAM_TRACKS): fr_stream_block_dense behind the call that makes every row live ------------------------
TRACKS_SCRIPT = [("prime", 0), ("begin",)] + [("dense", k) for k in range(1, 8)] + [("end",), ("begin",), ("dense", 8), ("dense", 9), ("end",), ("begin",),
                 ("dense", 10), ("dense", 11), ("dense", 12), ("end",), ("begin",), ("dense", 13), ("dense", 14), ("end",)]
TRACKS_STARTS = [(SEEK - 64, 64)] + [(SEEK + sum(K.FIRST_LENGTHS[:k]), K.FIRST_LENGTHS[k]) for k in range(7)] + [
    (FORWARD, 64), (FORWARD + 64, 37), (BACK, 64), (BACK + 64, 64), (BACK + 128, 22), (FAR_LOW, 64), (FAR_LOW + 64, 64)]


def _stream_tracks_case():
    """stream_tracks_cases' trk_128 (two track voices of 128 partials: 513 input rows): one fr_fill_buffer_dense for ceil(513 / 64)
    output slots makes every row live (the store keeps n_slots * n_times vectors), then streams of dense blocks: from B - 100
    across B, a seek forward, a seek back across B, the far seek."""
    import stream_tracks_cases as TK
    c = TK.case("trk_128")
    tree = c.build()
    n_in = c.n_in()
    prime_slots = -(-n_in // 64)

    def low():
        rng = np.random.default_rng(zlib.crc32(b"stream:trk_128"))
        return [(S0_VOICES + off, n, list(TK.matrix(c, 0, 0, time_row(off, n), k, rng))) for k, (off, n) in enumerate(TRACKS_STARTS)]

    def check(plan, k, T):
        st = plan["stream"]
        assert st["servable"] and st["kernel"] == TK.KERNEL and st["tracks"]["rows"] == n_in - 1, st

    return _case("stream:trk_128", "stream", S0_VOICES, lambda r: synth.install(r, tree), 2, dict(c.options), low, _voice_expected(tree, "reference"),
                 [], False, check, n_in, kind="mixed", script=TRACKS_SCRIPT, setup=lambda r: r.set_track_inputs(1), setup_needs_jit=True, prime_slots=prime_slots)


STAGE_CASES = [c for c in sv.CASES if c["seek"] is None and c["graph"][0] != "wide"]     # feed-forward, not `wide`
STREAM_CASES = [c for c in X.CASES if not c["feedback"]]

CASES = [_stage_case(c) for c in STAGE_CASES] + [_step_case("interpreter", {"FR_STAGE_JIT": "0"}, "stage_kernel/"),
                                                 _step_case("compiled", {"FR_STAGE_JIT": "force"}, "jit_stage[")] + [_pull_case()] + [
    _bank_case("short", 130, {}, "bank_short_kernel", V=2, P=512),
    _bank_case("long", 600, {"FR_BANK_SHORT": "0"}, "bank_kernel"),
    _bank_case("compiled", 600, {"FR_BANK_TEMPLATE": "0"}, "jit_bank"),
] + [_observed_case(), _ring_keep_case()] + _track_cases() + [_stream_case(c) for c in STREAM_CASES] + _more_stream_cases() + [_store_case(), _stream_tracks_case()]
FAMILIES = ["pull", "stage interpreter", "compiled stage", "bank to rings", "stream"]
# one case per family for PER_FAMILY's bases: the deepest look-back of each
FAMILY_CASE = {"pull": "pull:randgraph", "stage interpreter": "stage:stage_kernel/strided", "compiled stage": "stage:jit_stage[deep,P,B4]/strided",
               "bank to rings": "bank:long", "stream": "stream:taps_64_2x128"}


def case(name):
    for c in CASES:
        if c["name"] == name:
            return c
    raise KeyError(name)


_LOW = {}


def low_twin(name):
    """(low sequence, expected blocks) of a case: rendered once per process by the dense reference, and left unchanged."""
    if name not in _LOW:
        c = case(name)
        low = c["low"]()
        _LOW[name] = (low, c["expected"](low))
    return _LOW[name]


def nonzero_share(expected):
    """Per output row, the share of finite non-zero samples of a list of [n_rows, T] blocks."""
    a = np.concatenate(expected, axis=1)
    return (np.isfinite(a) & (a != 0)).mean(axis=1)


def run_calls(lib, c, calls, after=None):
    """The calls through fr_fill_buffer (or _dense) of one renderer of `lib` with the case's options; after(plan, k, T) per call.
    The simulator has no hipRTC, and only compiled leaves read tracks in place: a case with `setup_needs_jit` runs there
    without its setup (its tracks are then ordinary stored rows)."""
    from libfriendship_amd.capi import Renderer
    got = []
    with Renderer(lib, mode=c["mode"], semantics=c["semantics"], options=c["options"] or None) as r:
        sim = lib.path.endswith("libfr_simengine.so") or "simasan" in lib.path
        if "setup" in c and lib.backend != "cpu-oracle" and not (sim and c.get("setup_needs_jit")):   # (the oracle takes tracks as ordinary rows)
            c["setup"](r)
        c["install"](r)
        for k, (idx, T, rows) in enumerate(calls):
            if k in c.get("edits", {}):
                c["edits"][k](r)
            if c["entry"] == "dense":
                got.append(r.fill_buffer_dense(c["n_rows"], idx, idx + T, np.stack(rows)))
            else:
                got.append(r.fill_buffer(c["n_rows"], idx, idx + T, rows))
            if after:
                after(r.plan(), k, T)
    return got


def run_mixed(lib, c, calls, streamed=True, options=None, after=None):
    """A "mixed" case's script on one renderer: fr_fill_buffer calls, streams (streamed=False: their fr_fill_buffer twin) and the
    case's edit, over the sequence `calls`; returns the results in the sequence's order.  The script ends where `calls` does."""
    from libfriendship_amd.capi import Renderer
    got = [None] * len(calls)
    with Renderer(lib, semantics=c["semantics"], options=options) as r:
        sim = lib.path.endswith("libfr_simengine.so") or "simasan" in lib.path
        if "setup" in c and lib.backend != "cpu-oracle" and not (sim and c.get("setup_needs_jit")):
            c["setup"](r)
        c["install"](r)
        first_block = False
        for step in c["script"]:
            if len(step) > 1 and step[1] >= len(calls):
                break
            if step[0] == "edit":
                for apply in c["edits"].values():
                    apply(r)
            elif step[0] == "begin":
                first_block = True
                if streamed:
                    r.stream_begin(c["n_rows"])
            elif step[0] == "end":
                if streamed:
                    r.stream_end()
            else:
                k = step[1]
                idx, T, rows = calls[k]
                if step[0] in ("block", "dense") and streamed:
                    got[k] = r.stream_block_rows(idx, rows, n_times=T) if step[0] == "block" else r.stream_block_dense(idx, np.stack(rows))
                    if first_block:
                        c["check"](r.plan(), k, T)
                    first_block = False
                elif step[0] == "prime":                        # every input row becomes live: more output slots than the patch has rows
                    got[k] = r.fill_buffer_dense(c["prime_slots"], idx, idx + T, np.stack(rows))[:c["n_rows"]]
                else:
                    got[k] = r.fill_buffer(c["n_rows"], idx, idx + T, rows)
                    if after:
                        after(r.plan(), k, T)
        if streamed and step[0] != "end":
            r.stream_end()
    return got


def oracle_at(oracle_lib, c, calls, frames, row0=None):
    """The C++ oracle at (call, column) pairs of `calls`, all rows: {(call, column): float32 [n_rows]}.  The calls' rows go into
    its input store call by call -- it renders output row 0 meanwhile (appended to `row0`): the store keeps n_slots * n_times
    vectors, so a call for no row would store nothing --, and every frame is sought in the store's state after its call (fro_eval_samples)."""
    import oracle_tools
    from libfriendship_amd.capi import Renderer
    by_call = {}
    for k, col in frames:
        by_call.setdefault(k, []).append(col)
    out = {}
    with Renderer(oracle_lib, semantics=c["semantics"]) as o:
        c["install"](o)
        n_slots = max(1, -(-len(calls[0][2]) // calls[0][1]))          # (the first call makes every input row live)
        for k, (idx, T, rows) in enumerate(calls):
            if k in c.get("edits", {}):
                c["edits"][k](o)
            first = o.fill_buffer(n_slots, idx, idx + T, rows)
            if row0 is not None:
                row0.append(first[:1])
            cols = by_call.get(k, [])
            if cols:
                slots = np.repeat(np.arange(c["n_rows"], dtype=np.uint32), len(cols))
                times = np.tile(np.array([idx + col for col in cols], np.uint64), c["n_rows"])
                vals = oracle_tools.eval_samples(o, slots, times).reshape(c["n_rows"], len(cols))
                for j, col in enumerate(cols):
                    out[(k, col)] = vals[:, j]
    return out


def feedback_refusal(lib, options=None):
    """x = in0 + 0.5 * Delay(x, 3) on `lib`: a seek to 2^28 + 1 is refused with FR_ERR_UNSUPPORTED and the frame's number, and
    the seek to frame 300 after it is served: every sample of it and of the contiguous call behind it equals the dense reference."""
    from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, RenderError, Renderer
    g = sv.GRAPHS["echo"]((3,))
    rng = np.random.default_rng(28)
    frame = FB_MAX_REPLAY + 1
    store, ref = sr.InputStore(), sr.DenseReference(g)
    with Renderer(lib, options=options) as r:
        g.install(r)
        try:
            r.fill_buffer(1, frame, frame + 64, [rng.normal(size=64).astype(np.float32)])
        except RenderError as e:
            assert e.status == FR_ERR_UNSUPPORTED and str(frame) in str(e), e
        else:
            raise AssertionError(f"a feedback plan served a seek to frame {frame}")
        for idx, T in ((300, 64), (364, 130)):
            rows = [rng.normal(size=T).astype(np.float32)]
            store.call(idx, rows)
            got = r.fill_buffer(1, idx, idx + T, rows)
            assert r.plan()["feedback"]
            msg = sr.first_diff(got, ref(store, idx, idx + T), f"the call at {idx} after the refusal")
            assert not msg, msg
