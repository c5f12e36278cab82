"""Patches and call sequences for a stream that STORES what it is fed (FR_STREAM_STORE on top of FR_STREAM_PROGRAMS), shared by
the simulator tests (tests/test_stream_store_sim.py) and the GPU tests (tests/test_hip_stream_store.py).  Graph recipes and plain
data: importable without a GPU.

With the option the contract of fr_stream_* is: results and statuses are those of fr_fill_buffer for the same sequence of calls
AND EDITS, whatever mixture of fr_fill_buffer, edits and streams the host makes.  So a sequence here is a list of STEPS,
  ("fill", idx, T, rows)   fr_fill_buffer of [idx, idx + T)
  ("begin",) / ("end",)    fr_stream_begin / fr_stream_end
  ("block", idx, T, rows)  fr_stream_block_rows of [idx, idx + T); the rows may be short, empty or missing
  ("edit", name)           the patch's edit of that name (a function of a renderer)
and `run` plays it on a renderer either as written or -- `streamed=False` -- with every block as fr_fill_buffer and begin / end
as nothing: the twin the streamed results must equal bit for bit, statuses included.  `seek_at`: the twin makes a one-frame call
at frame 0 before the step of that number, so that step is a SEEK: what a stream's first block was before the option, and what a
case must be able to tell from continuing (tests/test_stream_store_sim.py proves it on the oracle).

The shapes are the smallest at which this can go wrong: 2 voices x 128 partials (the smallest chunked bank) and, with
FR_STREAM_GENERAL, one 32-partial schedule voice; a tap of 100 frames, a tap of 3 frames behind a bus, Delay(In(1), 70) on a
control row, combs of 441 and 5 frames, an echo on In(1) without a voice.  Block lengths are stream_cases.FIRST_LENGTHS."""
import zlib

import numpy as np

import stream_cases as K
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_OK, RenderError

NEW_KERNEL, NEW_FX_KERNEL = "bank_stream_store_kernel", "bank_stream_store_fx_kernel"
PROGRAMS = dict(K.OPTION)
STORE = dict(PROGRAMS, FR_STREAM_STORE="1")
IDLE = {"FR_STREAM_IDLE_MS": "1500"}
FINITE_SHARE = 0.95
LENGTHS = K.FIRST_LENGTHS                       # 64, 64, 1, 37, 64, 2, 63: 295 frames
CONST = synth.CONST_HANDLE
FAR = 0                                         # where the twin's seek-forcing call goes: one frame at 0, so the step after it is a seek


def f32_bits(x):
    return int(np.asarray(x, np.float32).view(np.uint32))


def swap_const(node, slot, old, new):
    def apply(r):
        r.on_del_edge(CONST, int(node), f32_bits(old), slot)
        r.on_add_edge(CONST, int(node), f32_bits(new), slot)
    return apply


class Patch:
    """A graph, its output rows, the input slots the host feeds, the options that serve it, and its edits by name."""

    def __init__(self, name, options, n_in, voiceless=False):
        self.name, self.options, self.n_in, self.voiceless = name, dict(options), n_in, voiceless
        self.g = synth.GraphArrays()
        self.edits, self.n_rows, self.tree = {}, 0, None
        # how much is rendered before a boundary: `fills` calls of 150 frames, `rounds` times the seven block lengths.  One of each
        # unless the patch's shortest delay reaches further back: then a seek at the boundary could not be told from continuing
        self.fills = self.rounds = 1

    def voices(self, V, P, seed=0x5EED0E00):
        p = synth.voice_params(V, P, seed, wrap=64)
        return synth.sum_tree(self.g, synth.partial_leaves(self.g, p["w"], p["amp"]).reshape(V, P))

    def rows(self, roots):
        roots = np.asarray(roots, dtype=np.uint32)
        self.g.edge(roots, 0, 0, np.arange(len(roots), dtype=np.uint32))
        self.n_rows = len(roots)
        self.tree = self.g.finish(self.n_rows)
        self.next = int(self.g.next)
        return self

    def install(self, r):
        synth.install(r, self.tree)


def tap_patch(V=2, P=128, options=PROGRAMS, name="tap_100", d=100.0, gain=0.5):
    """row v = gain * voice v + 0.5 * Delay(voice v, d).  Edits: `gain` (a constant), `longer` (the tap reads 150 frames back:
    frames streamed before the edit), `note_on` (one more voice of P partials on one more row) and `delay_in2` (row 0 becomes
    row 0 + Delay(In(2), 40): a slot the host fed all along and no program read)."""
    p = Patch(name, options, 3)
    g = p.g
    x = p.voices(V, P)
    dry = g.binop(synth.K_MUL, synth.C(np.float32(gain)), x, V)
    dl = g.binop(synth.K_DELAY, x, synth.C(np.float32(d)), V)
    y = g.binop(synth.K_SUM2, dry, g.binop(synth.K_MUL, synth.C(np.float32(0.5)), dl, V), V)
    p.rows(y)
    p.dry = dry                                  # (the gains' nodes: tools/stream_store_probe.py turns one back and forth)
    p.edits["gain"] = swap_const(dry[0], 0, gain, 0.8125)
    p.edits["longer"] = swap_const(dl[0], 1, d, 150.0)

    def note_on(r):
        g2 = synth.GraphArrays()
        g2.next, g2.handles, g2.kinds = p.next, [], []
        q = synth.voice_params(1, P, 0x5EED0E77, wrap=64)
        root = synth.sum_tree(g2, synth.partial_leaves(g2, q["w"], q["amp"]).reshape(1, P))
        d2 = g2.binop(synth.K_DELAY, root, synth.C(np.float32(d)), 1)
        y2 = g2.binop(synth.K_SUM2, root, g2.binop(synth.K_MUL, synth.C(np.float32(0.5)), d2, 1), 1)
        g2.edge(y2, 0, 0, V)
        synth.install(r, {"handles": np.concatenate(g2.handles), "kinds": np.concatenate(g2.kinds),
                          "edges": np.ascontiguousarray(np.concatenate(g2.edges, axis=0), dtype=np.uint32)})
    p.edits["note_on"] = note_on

    def delay_in2(r):
        h = p.next + 4096                        # (clear of a note-on's handles)
        r.on_add_node(h, "Delay")
        r.on_add_node(h + 1, "Sum2")
        r.on_add_edge(0, h, 2, 0)
        r.on_add_edge(CONST, h, f32_bits(40.0), 1)
        r.on_del_edge(int(y[0]), 0, 0, 0)
        r.on_add_edge(int(y[0]), h + 1, 0, 0)
        r.on_add_edge(h, h + 1, 0, 1)
        r.on_add_edge(h + 1, 0, 0, 0)
    p.edits["delay_in2"] = delay_in2
    p.rows_after = {"note_on": V + 1}
    return p


def bus_tap_patch(V=2, P=128):
    """row 0 = Delay(voice 0, 3) + Delay(voice 1, 3): short taps behind a bus; row 1 = voice 1 * c."""
    p = Patch("bus_tap_3", dict(PROGRAMS, FR_STREAM_BUS="1"), 1)
    g = p.g
    x = p.voices(V, P)
    a = g.binop(synth.K_DELAY, x[0:1], synth.C(np.float32(3.0)), 1)
    b = g.binop(synth.K_DELAY, x[1:2], synth.C(np.float32(3.0)), 1)
    m = g.binop(synth.K_MUL, synth.C(np.float32(0.75)), x[1:2], 1)
    p.rows(np.concatenate([g.binop(synth.K_SUM2, a, b, 1), m]))
    p.edits["gain"] = swap_const(m[0], 0, 0.75, 0.3125)
    return p


def control_patch(V=2, P=128):
    """row v = voice v * Delay(In(1), 70): a delayed control row."""
    p = Patch("control_70", dict(PROGRAMS, FR_STREAM_INPUTS="1", FR_STREAM_HISTORY="1"), 2)
    g = p.g
    x = p.voices(V, P)
    dl = g.binop(synth.K_DELAY, synth.IN(1), synth.C(np.float32(70.0)), 1)
    sc = g.binop(synth.K_MUL, dl, synth.C(np.float32(0.5)), 1)
    y = g.binop(synth.K_MUL, x, np.repeat(sc, V), V)
    p.rows(y)
    p.edits["gain"] = swap_const(sc[0], 1, 0.5, 0.8125)
    return p


def deep_control_patch(V=2, P=128):
    """row v = voice v * 0.5 * (Delay(In(1), 70) + Delay(In(1), 250)): the long stretches' patch.  Its deeper read reaches back
    over the frame at which a slot's buffer slides or doubles, from the blocks behind that frame and from the fr_fill_buffer call
    that follows the stream; 250 frames stay within a bounded history of HISTORY_FRAMES."""
    p = Patch("control_70_250", dict(PROGRAMS, FR_STREAM_INPUTS="1", FR_STREAM_HISTORY="1"), 2)
    g = p.g
    x = p.voices(V, P)
    a = g.binop(synth.K_DELAY, synth.IN(1), synth.C(np.float32(70.0)), 1)
    b = g.binop(synth.K_DELAY, synth.IN(1), synth.C(np.float32(250.0)), 1)
    sc = g.binop(synth.K_MUL, g.binop(synth.K_SUM2, a, b, 1), synth.C(np.float32(0.5)), 1)
    p.rows(g.binop(synth.K_MUL, x, np.repeat(sc, V), V))
    return p


def late_slots_patch(P=128, slot=2):
    """ONE row = voice * In(slot) + 0.5 * Delay(In(slot), 40): the plan reads the slots 0 and `slot`, and with one output row the
    input vectors are as many as the longest block so far has frames -- a slot comes into being, and can be fed, with the first
    block that is long enough."""
    p = Patch(f"late_slots_{slot}", dict(PROGRAMS, FR_STREAM_INPUTS="1", FR_STREAM_HISTORY="1"), 3)
    g = p.g
    x = p.voices(1, P)
    dl = g.binop(synth.K_DELAY, synth.IN(slot), synth.C(np.float32(40.0)), 1)
    wet = g.binop(synth.K_MUL, dl, synth.C(np.float32(0.5)), 1)
    p.rows(g.binop(synth.K_SUM2, g.binop(synth.K_MUL, x, synth.IN(slot), 1), wet, 1))
    return p


def comb_patch(d, V=2, P=128):
    """row v = x_v = voice v + 0.6 * Delay(x_v, d).  The edit turns voice 0's feedback gain: the loop itself changes."""
    options = PROGRAMS if d >= 64 else dict(PROGRAMS, FR_STREAM_LOOPS="1")
    p = Patch(f"comb_{d}", options, 1)
    g = p.g
    roots = p.voices(V, P)
    x = g.nodes(synth.K_SUM2, V)
    dl = g.binop(synth.K_DELAY, x, synth.C(np.float32(d)), V)
    m = g.binop(synth.K_MUL, dl, synth.C(np.float32(0.6)), V)
    g.edge(roots, x, 0, 0)
    g.edge(m, x, 0, 1)
    p.rows(x)
    p.edits["gain"] = swap_const(m[0], 1, 0.6, 0.4375)
    if d >= 150:                                 # (the loop has to have come round before the boundary)
        p.fills, p.rounds = d // 150 + 2, d // 295 + 1
    return p


def echo_patch(d=100):
    """row 0 = x = In(1) + 0.5 * Delay(x, d): no voice at all.  The edit turns the feedback gain."""
    p = Patch("echo_in1", dict(PROGRAMS, FR_STREAM_EFFECTS="1", FR_STREAM_INPUTS="1"), 2, voiceless=True)
    g = p.g
    dl = g.nodes(synth.K_DELAY, 1)
    g.const(dl, np.float32(d), 1)
    m = g.binop(synth.K_MUL, dl, synth.C(np.float32(0.5)), 1)
    x = g.binop(synth.K_SUM2, synth.IN(1), m, 1)
    g.edge(x, dl, 0, 0)
    p.rows(x)
    p.edits["gain"] = swap_const(m[0], 1, 0.5, 0.4375)
    return p


PATCHES = {
    "tap_100": tap_patch,
    "tap_100_general_1x32": lambda: tap_patch(1, 32, dict(PROGRAMS, FR_STREAM_GENERAL="1"), "tap_100_general_1x32"),
    "bus_tap_3": bus_tap_patch,
    "control_70": control_patch,
    "comb_441": lambda: comb_patch(441),
    "comb_5": lambda: comb_patch(5),
    "echo_in1": echo_patch,
}
# the edits that need more than the patch's own options: the new Delay(In(2), 40) reads an input row at a delay
EDIT_OPTIONS = {"delay_in2": {"FR_STREAM_INPUTS": "1", "FR_STREAM_HISTORY": "1"}, "note_on": {"FR_STREAM_BANKS": "1"}}


def rows_at(name, n_in, idx, T):
    """The block's full rows: the time ramp and control rows in [0.5, 1.5), a function of the patch's name and the frame."""
    rows = [synth.time_ramp(idx, idx + T)]
    for s in range(1, n_in):
        rng = np.random.default_rng([zlib.crc32(name.encode()), s, idx])
        rows.append(rng.uniform(0.5, 1.5, size=T).astype(np.float32))
    return rows


def blocks_from(name, n_in, idx, n=len(LENGTHS)):
    """n consecutive blocks from idx with the lengths of stream_cases.FIRST_LENGTHS: [("block", idx, T, rows)]."""
    out = []
    for k in range(n):
        T = LENGTHS[k % len(LENGTHS)]
        out.append(("block", idx, T, rows_at(name, n_in, idx, T)))
        idx += T
    return out, idx


# ---- the sequences ---------------------------------------------------------------------------------------------------------------
# Each returns (steps, boundaries): `boundaries` are the numbers of the steps that are the first rendered after a boundary --
# fr_fill_buffer -> stream, stream -> edit -> stream, stream -> fr_fill_buffer -- where the option makes a continuation of what
# was a seek.

def seq_fill_then_stream(p):
    """1. fr_fill_buffer of 150 frames from 0 (comb_441: four such calls), then a stream continuing where it ended."""
    steps = [("fill", 150 * k, 150, rows_at(p.name, p.n_in, 150 * k, 150)) for k in range(p.fills)] + [("begin",)]
    blocks, _ = blocks_from(p.name, p.n_in, 150 * p.fills)
    return steps + blocks + [("end",)], [len(steps)]


def seq_stream_edit_stream(p, edit="gain"):
    """2. a stream from 0, an edit, a stream continuing."""
    first, at = blocks_from(p.name, p.n_in, 0, len(LENGTHS) * p.rounds)
    second, _ = blocks_from(p.name, p.n_in, at)
    steps = [("begin",)] + first + [("end",), ("edit", edit), ("begin",)]
    return steps + second + [("end",)], [len(steps)]


def seq_stream_then_fill(p):
    """3. a stream from 0, then fr_fill_buffer continuing: its taps read into streamed frames."""
    first, at = blocks_from(p.name, p.n_in, 0, len(LENGTHS) * p.rounds)
    steps = [("begin",)] + first
    return steps + [("fill", at, 150, rows_at(p.name, p.n_in, at, 150)), ("fill", at + 150, 64, rows_at(p.name, p.n_in, at + 150, 64))], [len(steps)]


def seq_seeks(p):
    """4. a seek forward and a seek back inside one stream: still seeks."""
    a, _ = blocks_from(p.name, p.n_in, 0)
    b, _ = blocks_from(p.name, p.n_in, 5003, 3)
    c, _ = blocks_from(p.name, p.n_in, 69, 3)
    return [("begin",)] + a + b + c + [("end",)], []


def seq_row_rules(p):
    """5. the store's row rules across a boundary (a patch with a control row in slot 1): fr_fill_buffer stores a short row; the
    first streamed block brings an EMPTY row for slot 1, padded with the value fr_fill_buffer stored last; then slot 1 gets no row
    for two blocks and lags; the fr_fill_buffer that follows leaves it out too, and the one after that feeds it again: the status
    is the reference's, FR_ERR_INPUT_HISTORY."""
    assert p.n_in == 2
    r = rows_at(p.name, 2, 0, 150)
    steps = [("fill", 0, 150, [r[0], r[1][:97]]), ("begin",)]
    idx = 150
    for k, kind in enumerate(("empty", "full", "short", "none", "none")):
        T = LENGTHS[k]
        rows = rows_at(p.name, 2, idx, T)
        rows = {"empty": [rows[0], rows[1][:0]], "full": rows, "short": [rows[0], rows[1][:max(T // 2, 1)]], "none": rows[:1]}[kind]
        steps.append(("block", idx, T, rows))
        idx += T
    steps.append(("fill", idx, 64, rows_at(p.name, 2, idx, 64)[:1]))
    steps.append(("fill", idx + 64, 64, rows_at(p.name, 2, idx + 64, 64)))   # slot 1 lags: refused as fr_fill_buffer refuses it
    return steps, [2]


def seq_late_slots(p, too_many=False):
    """A stream whose second block feeds two slots more, one of them (slot 1) below a slot the launch already streams (slot 2, which
    the plan reads): the set of streamed slots grows, the doorbell's rows change places, the programs are uploaded again -- a
    relaunch, not a seek.  Then blocks of every length, the stream's end and fr_fill_buffer continuing, its Delay(In(2), 40)
    reading streamed frames.  `too_many`: before the second block one with NINE rows, which is refused (FR_ERR_UNSUPPORTED) and
    leaves no trace."""
    steps = [("begin",), ("block", 0, 1, rows_at(p.name, 1, 0, 1))]
    if too_many:
        steps.append(("block", 1, 64, rows_at(p.name, 9, 1, 64)))
    idx = 1
    for T in LENGTHS:
        steps.append(("block", idx, T, rows_at(p.name, 3, idx, T)))
        idx += T
    return steps + [("end",), ("fill", idx, 150, rows_at(p.name, 3, idx, 150))]


LATE_SHORT_BLOCKS = 60


def seq_late_third(p):
    """A stream of a patch that reads the slots 0 and 1: 60 blocks of two frames, which feed both, then a full block that also
    feeds slot 2.  The set grows in the middle of the stream, the stream's history is filled again from the store, and
    Delay(In(1), 40) reads it across the relaunch."""
    steps, idx = [("begin",)], 0
    for _ in range(LATE_SHORT_BLOCKS):
        steps.append(("block", idx, 2, rows_at(p.name, 2, idx, 2)))
        idx += 2
    for T in LENGTHS:
        steps.append(("block", idx, T, rows_at(p.name, 3, idx, T)))
        idx += T
    return steps + [("end",), ("fill", idx, 150, rows_at(p.name, 3, idx, 150))]


def run(r, p, steps, streamed=True, seek_at=(), n_rows=None):
    """Plays `steps` on renderer `r` (the patch installed by the caller); returns [(status, array or None)] for every fill and
    block step, in order.  `streamed=False`: the fr_fill_buffer twin.  `on_block`: called after every streamed block."""
    out = []
    n_rows = p.n_rows if n_rows is None else n_rows
    for k, s in enumerate(steps):
        if k in seek_at:
            assert not streamed
            r.fill_buffer(n_rows, FAR, FAR + 1, [])
        if s[0] == "edit":
            p.edits[s[1]](r)
            n_rows = getattr(p, "rows_after", {}).get(s[1], n_rows)
        elif s[0] == "begin":
            if streamed:
                r.stream_begin(n_rows)
        elif s[0] == "end":
            if streamed:
                r.stream_end()
        else:
            _, idx, T, rows = s
            try:
                if s[0] == "block" and streamed:
                    out.append((FR_OK, r.stream_block_rows(idx, rows, n_times=T)))
                else:
                    out.append((FR_OK, r.fill_buffer(n_rows, idx, idx + T, rows)))
            except RenderError as e:
                out.append((e.status, None))
    return out


def rendered_steps(steps):
    """The numbers of the steps that render (fill, block), in order: the k-th result of `run` is of step rendered_steps[k]."""
    return [k for k, s in enumerate(steps) if s[0] in ("fill", "block")]


# (sequence name, patch, builder, edit)
SEQUENCES = (
    [("fill_then_stream", n, seq_fill_then_stream, None) for n in PATCHES] +
    [("stream_edit_stream", n, seq_stream_edit_stream, "gain") for n in PATCHES] +
    [("stream_edit_stream", "tap_100", seq_stream_edit_stream, e) for e in ("longer", "note_on", "delay_in2")] +
    [("stream_then_fill", n, seq_stream_then_fill, None) for n in PATCHES] +
    [("seeks", n, seq_seeks, None) for n in PATCHES] +
    [("row_rules", n, seq_row_rules, None) for n in ("control_70", "echo_in1")]
)


def sequence_id(s):
    return f"{s[0]}-{s[1]}" + (f"-{s[3]}" if s[3] and s[3] != "gain" else "")


def build(s):
    """(patch, steps, boundaries, options) of an entry of SEQUENCES."""
    seq, name, f, edit = s
    p = PATCHES[name]()
    steps, bounds = f(p, edit) if edit else f(p)
    return p, steps, bounds, dict(p.options, **EDIT_OPTIONS.get(edit, {}))


# ---- the long stretches: a slide of a bounded history, a doubling of an unbounded one ------------------------------------------------
HISTORY_FRAMES = 256
# A slot's buffer is max(2 * (keep + block), 65536) frames with a bounded history and 2^20 without: block 1024 is the first that
# does not fit the one, block 16384 the other, and the launch is relaunched with it.  The streams end THREE blocks later, so that the
# last 8 blocks, which are compared, straddle the relaunch -- the blocks behind it read the stream's history 250 frames back, into
# frames streamed before it -- and the fr_fill_buffer call that follows the stream reads the STORE 250 frames back, over that frame.
SLIDE_BLOCK, DOUBLING_BLOCK = 65536 // 64, (1 << 20) // 64
SLIDE_FRAMES = (SLIDE_BLOCK + 3) * 64           # 1027 blocks
DOUBLING_FRAMES = (DOUBLING_BLOCK + 3) * 64     # 16387 blocks
LONG_CALL = 4800
COMPARED = 8


def long_stretch(frames):
    """[(idx, T)] of full blocks over [0, frames) and the number of the first of the last COMPARED."""
    n = frames // 64
    return [(k * 64, 64) for k in range(n)], n - COMPARED
