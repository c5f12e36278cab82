"""Patches for block streaming of feedback loops through Delays of a SIGNAL amount (FR_STREAM_SWEEP on top of FR_STREAM_PROGRAMS,
FR_STREAM_LOOPS and FR_STREAM_DYN; csrc/streamplan.hpp), shared by the simulator tests of the serving rule
(tests/test_stream_sweep_sim.py) and the GPU tests of the four sweep kernels (tests/test_hip_stream_sweep.py).  Graph recipes and
plain data: importable without a GPU.

The graphs are those of tests/loop_dyn_cases.py (FR_LOOP_DYN), the block lengths stream_cases.finite_block_rows'.  Expectations
come from the graph:
  * `widths`: the nonzero entries of stream.sweep_programs, sorted -- a sweep program's width is the least number of frames a read
    of its own rings reaches back: the proven lower bound of the amount (loop_dyn_cases: floor(base) - 1 for a whole base), or a
    constant tap below it; at a bound of 64 the program is no sweep program and keeps the kernel it had;
  * `strides`: the nonzero entries of stream.loop_programs, sorted: the widths, and the strides of constant loops;
  * rule (b), `tap_behind`: the second row's program reads the flanger's ring through a Delay that may reach 0 frames back and
    follows it into the same segment; rule (c), `chorus_comb`: a comb of 8 frames whose input is the voice delayed by 4 * lfo --
    one loop program of stride 8 that holds an S_READ_DYN of the bank's ring (the planner inlines it: stream.dyn_reads counts it).

Conditions on the inputs: a NaN that enters a loop stays.  The audio row in0 is finite noise and the voices' time row is
finite_block_rows'; hostile values -- NaN, infinities, -0, subnormals, huge -- go into the LFO / knob row of the voiceless cases
alone, where Minimum(c, .) with the constant on the left keeps the amount finite."""
import numpy as np

import loop_dyn_cases as L
import stage_variants as sv
import stream_cases as K
import stream_fx_cases as FX
import stream_loop_cases as SL
from libfriendship_amd import synth

KERNELS = {(False, False): "bank_stream_sweep_kernel", (True, False): "bank_stream_sweep_fx_kernel",
           (False, True): "bank_stream_sweep_store_kernel", (True, True): "bank_stream_sweep_store_fx_kernel"}
LOOP_DYN = {"FR_LOOP_DYN": "1"}                                   # the fr_fill_buffer twin: no stream option
VOICES = dict(LOOP_DYN, FR_STREAM_PROGRAMS="1", FR_STREAM_LOOPS="1", FR_STREAM_DYN="1", FR_STREAM_SWEEP="1")
VOICELESS = dict(VOICES, FR_STREAM_EFFECTS="1", FR_STREAM_INPUTS="1")
IDLE = dict(SL.IDLE)
FINITE_SHARE = 0.95
LOUD = 0.01
FRAMES = 1500
OLD_SWEEP_REASON = "a feedback loop delays by a signal amount (a sweep plan, FR_LOOP_DYN): block streaming does not serve it"
OLD_LOOP_REASON = ("a loop program uses S_READ_DYN (a Delay by a signal amount inside a feedback loop shorter than a block), which block streaming does not "
                   "serve yet")
GAIN, NEW_GAIN = 0.5, 0.4375                                      # the store cases' edit


def chorus_comb_tree(V, P, d=8, depth=4.0, rate=0.01, gain=0.6):
    """x = Delay(voice, depth * lfo(t)) + gain * Delay(x, d): a chorus into a comb -- rule (c)."""
    g = synth.GraphArrays()
    f = np.float32
    v = SL._voices(g, V, P)
    ramp = g.binop(synth.K_MOD, g.binop(synth.K_MUL, synth.IN(0), synth.C(f(rate)), 1), synth.C(f(1.0)), 1)
    amt = g.binop(synth.K_MUL, synth.C(f(depth)), g.binop(synth.K_MIN, synth.C(f(1.0)), ramp, 1), 1)
    wet = g.nodes(synth.K_DELAY, V)
    g.edge(v, wet, 0, 0)
    g.edge(np.broadcast_to(amt, (V,)), wet, 0, 1)
    x = g.nodes(synth.K_SUM2, V)
    dl = g.nodes(synth.K_DELAY, V)
    g.const(dl, f(d), 1)
    g.edge(x, dl, 0, 0)
    g.edge(wet, x, 0, 0)
    g.edge(g.binop(synth.K_MUL, dl, synth.C(f(gain)), V), x, 0, 1)
    g.edge(x, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


class Patch:
    """A case: the graph (a stage_reference.Graph for the voiceless cases, a synth tree for those with voices), how to install and
    edit it, and what fr_plan_json["stream"] must say."""

    def __init__(self, name, graph=None, tree=None, n_rows=1, n_in=2, widths=(), strides=None, per=(1,), oracle=600, knob_row=False,
                 semantics="reference", sweep_kernel=True, dyn_reads=None):
        self.name, self.graph, self.tree, self.n_rows, self.n_in = name, graph, tree, n_rows, n_in
        self.widths = sorted(widths)
        self.strides = sorted(self.widths if strides is None else strides)
        self.per, self.oracle, self.knob_row, self.semantics = sorted(per), oracle, knob_row, semantics
        self.voiceless = graph is not None
        self.options = dict(VOICELESS if self.voiceless else VOICES)
        self.sweep_kernel = sweep_kernel
        self.dyn_reads = dyn_reads

    def build(self):
        return self.graph() if self.voiceless else self.tree()

    def install(self, r, built=None):
        built = self.build() if built is None else built
        if self.voiceless:
            built.install(r)
        else:
            synth.install(r, built)
        return built

    def kernel(self, store=False):
        if not self.sweep_kernel:
            return "bank_stream_store_fx_kernel" if store else FX.NEW_KERNEL
        return KERNELS[(self.voiceless, store)]

    def gain_nodes(self, built):
        """The Multiply nodes whose constant is the loops' feedback gain (GAIN on input 1)."""
        bits = synth.bits(np.float32(GAIN))
        if self.voiceless:
            return [to for frm, to, fs, ts in built.edges if frm == 1 and fs == int(bits) and ts == 1 and built.nodes[to] == "Multiply"]
        e = built["edges"]
        return [int(h) for h in e[(e[:, 0] == synth.CONST_HANDLE) & (e[:, 2] == bits) & (e[:, 3] == 1), 1]]

    def edit_gain(self, r, built):
        """Turns the first loop's feedback gain from GAIN to NEW_GAIN: the loop itself changes."""
        nodes = self.gain_nodes(built)
        assert len(nodes) == (1 if self.voiceless else self.n_rows), nodes
        r.on_del_edge(synth.CONST_HANDLE, nodes[0], int(synth.bits(np.float32(GAIN))), 1)
        r.on_add_edge(synth.CONST_HANDLE, nodes[0], int(synth.bits(np.float32(NEW_GAIN))), 1)


def _fx(name, graph, args, widths, **kw):
    return Patch(name, graph=lambda: L.GRAPHS[graph](*args), widths=widths, **kw)


SERVABLE = [
    _fx("flanger_2_3", "flanger", (2.0, 3.0), [1]),
    _fx("flanger_8", "flanger", (8.0,), [7]),
    _fx("flanger_64", "flanger", (64.0,), [63]),
    # the bound is 64: no read reaches into a block, the program runs lane = frame and the plan keeps bank_stream_fx_kernel
    _fx("flanger_64_5", "flanger", (64.5,), [], sweep_kernel=False),
    _fx("knob", "knob", (), [2], knob_row=True),
    # two programs in a circle, merged into one that stores both rings; the second row is a copy of the second ring
    _fx("two_nodes", "two_nodes", (), [3], n_rows=2, per=(2,)),
    _fx("second_tap", "second_tap", (), [1], oracle=48),
    _fx("self_modulated", "self_modulated", (), [1], oracle=48, n_in=1),
    _fx("tap_behind", "tap_behind", (), [7], n_rows=2, per=(2,)),
    Patch("voices_base_8", tree=lambda: synth.feedback_flanger(2, 128, 8.0, 6.0, 0.01, GAIN), n_rows=2, n_in=1, widths=[7, 7], per=(1, 1)),
    Patch("voices_base_2", tree=lambda: synth.feedback_flanger(2, 128, 2.0, 3.0, 0.01, GAIN), n_rows=2, n_in=1, widths=[1, 1], per=(1, 1)),
    Patch("chorus_comb", tree=lambda: chorus_comb_tree(2, 128), n_rows=2, n_in=1, widths=[], strides=[8, 8], per=(1, 1), dyn_reads=2),
]
IDS = [p.name for p in SERVABLE]
STORE_CASES = ["flanger_8", "voices_base_8"]
SEEK_CASES = ["flanger_2_3", "flanger_8"]                          # w = 1 and 7
SEEKS = [(0, 300), (9000, 200), (2500, 200)]
WRAP_FRAMES = 33500


def case(name):
    for p in SERVABLE:
        if p.name == name:
            return p
    raise KeyError(name)


def without(options, *keys):
    return {k: v for k, v in options.items() if k not in keys}


def check_stream_object(s, p, store=False):
    """fr_plan_json["stream"] of a servable case against the graph's expectations."""
    assert s["servable"] is True and s["reason"] == "", (p.name, s)
    assert s["kernel"] == p.kernel(store), (p.name, s)
    assert sorted(w for w in s["sweep_programs"] if w) == p.widths, (p.name, s)
    assert sorted(l for l in s["loop_programs"] if l) == p.strides, (p.name, s)
    assert len(s["sweep_programs"]) == len(s["loop_programs"]) == sum(s["programs_per_voice"]) + s["bus_programs"], (p.name, s)
    assert all(w == 0 or w == l for w, l in zip(s["sweep_programs"], s["loop_programs"])), (p.name, s)    # a width stands where the stride stands
    assert sorted(s["programs_per_voice"]) == p.per and s["bus_programs"] == 0, (p.name, s)
    assert s["input_slots"] == list(range(p.n_in)), (p.name, s)
    if p.dyn_reads is not None:
        assert s["dyn_reads"] == p.dyn_reads, (p.name, s)


def lfo_row(p, base, k, rng):
    """The LFO / knob row of a voiceless case over a block: the frame ramp as finite_block_rows left it (its special values
    included), a knob row for the knob case; every third block carries every hostile kind in a third of its entries."""
    row = np.array(base, np.float32)
    if p.knob_row:
        row = np.resize(L.KNOB, len(row)).astype(np.float32)
        row[::7] = (rng.random(len(row[::7])) * 12 - 3).astype(np.float32)
    if k % 3 == 2:
        row[1::3] = np.resize(sv.HOSTILE, len(row[1::3]))
    return row


def blocks_of(p, starts, seed=23):
    """[(idx, T, rows)]: finite_block_rows' blocks over `starts` = [(first frame, frames)].  With voices: its time row.  Voiceless:
    in0 = finite noise, in1 = lfo_row."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (idx, t) in enumerate(SL.finite_block_rows(rng, starts)):
        T = len(t)
        if not p.voiceless:
            out.append((idx, T, [t]))
            continue
        in0 = (rng.normal(size=T) * 3).astype(np.float32)
        out.append((idx, T, [in0, lfo_row(p, t, k, rng)][:p.n_in]))
    return out


def short_blocks_of(p, seed=29):
    """Blocks of 64, 1 and 37 frames from frame 0 (stream_cases.short_blocks' lengths)."""
    rng = np.random.default_rng(seed)
    out = []
    for idx, t in SL.short_blocks(0):
        T = len(t)
        out.append((idx, T, [t] if not p.voiceless else [(rng.normal(size=T) * 3).astype(np.float32), np.array(t, np.float32)][:p.n_in]))
    return out


def concat_rows(blocks):
    """The rows of consecutive blocks from frame 0, joined: what one call over all of them would be fed."""
    assert blocks[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
    return [np.concatenate([rows[s] for _, _, rows in blocks]) for s in range(len(blocks[0][2]))]


_DENSE = {}


def dense_reference(p, blocks, key):
    """The dense forward reference (tests/loop_dyn_reference.py) of a voiceless case over consecutive blocks from frame 0, every
    frame; computed once per `key` and left unchanged."""
    if (p.name, key) not in _DENSE:
        import loop_dyn_reference as ldr
        rows = concat_rows(blocks)
        exp = ldr.render(p.build(), rows, 0, len(rows[0]), p.semantics)
        exp.setflags(write=False)
        _DENSE[(p.name, key)] = exp
    return _DENSE[(p.name, key)]


def condition_message(p, exp):
    """'' when every row of `exp` is at least FINITE_SHARE finite and louder than LOUD somewhere."""
    for r, row in enumerate(np.asarray(exp)):
        fin = np.isfinite(row)
        if fin.mean() < FINITE_SHARE:
            return f"{p.name}: row {r} is {fin.mean():.3f} finite, below {FINITE_SHARE}"
        if not (np.abs(row[fin]).max() > LOUD):
            return f"{p.name}: row {r} never exceeds {LOUD}"
    return ""


def stream_blocks(lib, p, blocks, options=None, semantics=None, edit_before=None):
    """The blocks through fr_stream_block_rows of one renderer; `edit_before`: the block before which the stream is closed, the gain
    edited and a stream begun again (a store stream: it continues at the renderer's head).  Returns the blocks' results and the "stream" objects read after the first block and at the end."""
    from libfriendship_amd.capi import Renderer
    with Renderer(lib, semantics=semantics or p.semantics, options=dict(p.options if options is None else options, **IDLE)) as s:
        built = p.install(s)
        s.stream_begin(p.n_rows)
        got, first = [], None
        for k, (idx, T, rows) in enumerate(blocks):
            if edit_before is not None and k == edit_before:     # (any other call closes a stream: end, edit, begin -- which continues)
                s.stream_end()
                p.edit_gain(s, built)
                s.stream_begin(p.n_rows)
            got.append(s.stream_block_rows(idx, rows, n_times=T))
            if k == 0:
                first = s.plan()["stream"]
            if edit_before is not None and k == edit_before:
                assert s.plan()["stream"]["store"]["continued"] is True, s.plan()["stream"]
        last = s.plan()["stream"]
        s.stream_end()
    return got, first, last


def fill_blocks(lib, p, blocks, semantics=None, edit_before=None, options=LOOP_DYN):
    """The same blocks (and the same edit) through fr_fill_buffer of a renderer with FR_LOOP_DYN=1 and no stream option."""
    from libfriendship_amd.capi import Renderer
    with Renderer(lib, semantics=semantics or p.semantics, options=dict(options)) as f:
        built = p.install(f)
        out = []
        for k, (idx, T, rows) in enumerate(blocks):
            if edit_before is not None and k == edit_before:
                p.edit_gain(f, built)
            out.append(f.fill_buffer(p.n_rows, idx, idx + T, rows))
    return out


def compare_blocks(got, exp, blocks, what):
    """Every sample of every block equal bit for bit (NaN = NaN, +0 != -0); returns the frames compared."""
    n = 0
    for k, ((idx, T, _), a, b) in enumerate(zip(blocks, got, exp)):
        assert K.same_bits(a, b), f"{what}: block {k} at frame {idx} (T={T}): " + K.first_diff(a, b)
        n += T
    return n
