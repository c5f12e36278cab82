"""Patches for block streaming of short and signal delays of COMPUTED values (FR_STREAM_TAPS on top of FR_STREAM_PROGRAMS), shared by
the simulator tests of the serving rule (tests/test_stream_taps_sim.py) and the GPU tests of the resident kernels
(tests/test_hip_stream_taps.py).  Graph recipes and plain data: importable without a GPU.

"Envelope, then effect": e = env * voice is a stage program of its own, and Delay(e, d) with d below a block -- or a signal amount
-- reads e's ring in the block that stores it.  Such a plan has no fused form; with the option it is served in its LEVEL FORM, every
level's programs in level order, and a reader follows its storer's voice (a plan without a voice: its group); one that would
follow two is a bus program.  The shapes are the smallest at which the kernel can go wrong:
  * env_fir_2x128: one hop at d = 1, one workgroup per voice;
  * env_taps_2x512: three levels, delays 63 and 64 on either side of the block, four chunks per voice -- the voice's finisher changes
    CU between blocks, so a program's ring is read across CUs and across blocks;
  * env_chorus_2x128: a signal amount that sweeps [0, 70): 0 frames, the same block, an earlier block;
  * bus_chorus_3x128, bus_fir_3x128: a bus program reading a bus program (S_READ_DYN in the bus segment; a chain of three and a
    row of a non-sink);
  * fx_product_delay, fx_product_knob_delay: stream_fx_cases' two refused patches without a voice;
  * general_env_fir_2x96: voices of 96 partials (FR_STREAM_GENERAL): a schedule bank under the same programs.
COMPOSED adds two that put the option next to the two serving options no case above sets: env_fir_gate_2x128 (FR_STREAM_HISTORY: a
delayed control row next to the tap, the hist kernel) and env_fir_beside_dry (FR_STREAM_BANKS: a dry voice of 512 partials in a
second bank, the bank table).  fx_product_knob_delay's amount row is knob_amounts: mostly inside (0, 48), fractional, with 0 and the
bound hit every 16 frames, so that one frame more of it changes most samples (tests/test_stream_taps_sim.py proves at least half).
Expectations come from the graph: the kernel (the launch rule's cascade), the levels, the reads below a block of rings that
programs store (`short`), of which signal reads (`dyn_ring`), the programs of each voice, the bus programs, the segments.

A case's sequence is stream_hist_cases.STREAMS: two streams on one renderer, 12 blocks with a seek forward to frame 5003 and a seek
back to frame 69, then a second stream from frame 0.  The first blocks have stream_cases.FIRST_LENGTHS, the 1-frame and 2-frame
blocks among them, after which a 63-frame read spans three blocks."""
import numpy as np

import stream_dyn_cases as D
import stream_fx_cases as F
import stream_hist_cases as H
import stream_loop_cases as L
from libfriendship_amd import synth

NEW_KEYS = ("levels", "short_reads", "dyn_ring_reads")
PROGRAMS = dict(H.PROGRAMS)                                     # FR_STREAM_PROGRAMS alone
OPTION = dict(PROGRAMS, FR_STREAM_TAPS="1")
DYN = dict(OPTION, FR_STREAM_DYN="1")
BUS = dict(OPTION, FR_STREAM_BUS="1")
BUS_DYN = dict(BUS, FR_STREAM_DYN="1")
GENERAL = dict(OPTION, FR_STREAM_GENERAL="1")
FX = dict(OPTION, FR_STREAM_EFFECTS="1", FR_STREAM_INPUTS="1")
FX_DYN = dict(FX, FR_STREAM_DYN="1")
# every serving option there was before this one (stream_fx_cases refuses its two patches with these)
ALL_BEFORE = dict(PROGRAMS, FR_STREAM_BUS="1", FR_STREAM_INPUTS="1", FR_STREAM_BANKS="1", FR_STREAM_LOOPS="1", FR_STREAM_GENERAL="1", FR_STREAM_DYN="1",
                  FR_STREAM_HISTORY="1", FR_STREAM_EFFECTS="1")
IDLE = dict(L.IDLE)
FINITE_SHARE = H.FINITE_SHARE
SENSITIVITY = H.SENSITIVITY
SIGNAL_SENSITIVITY = 0.5                                        # share of a row's finite samples that one more frame of a signal amount's base must change
STREAMS = H.STREAMS
NO_FUSED_FORM = F.NO_FUSED_FORM
DYN_OF_A_PROGRAM = F.DYN_OF_A_PROGRAM
MIX_BUS = "a program reads voices 0 and 1 in the same block (a mix bus across voices); each streamed program follows one voice"
CHORUS_DEPTH = 70.0
NAMED_BY_LAUNCH = ("bank_stream_prog_kernel", "bank_stream_bus_kernel")


def _enveloped(g, V, P, seed=0x5EED0E00):
    """e_v = env * voice_v: the ADSR (attack 48 frames, so the streams' first frames are on its slope) in front of every voice."""
    v = D._voices(g, V, P, seed)
    env = synth.adsr_envelope(g, attack=48.0, decay=120.0, sustain=0.6, release=4800.0, t_end=48000.0)
    return g.binop(synth.K_MUL, np.broadcast_to(env, v.shape), v, V)


def _tap(g, x, d, gain=None):
    """x + gain * Delay(x, d) (gain None: x + Delay(x, d))."""
    n = len(x)
    dl = g.binop(synth.K_DELAY, x, synth.C(np.float32(d)), n)
    if gain is not None:
        dl = g.binop(synth.K_MUL, synth.C(np.float32(gain)), dl, n)
    return g.binop(synth.K_SUM2, x, dl, n)


def _sweep(g, n, base=0.0, depth=CHORUS_DEPTH):
    """base + depth * Modulo(t * (v + 1) / 97, 1), v = 0 .. n-1: the amount sweeps [base, base + depth) every 97 / (v + 1) frames."""
    f = np.float32
    rates = (np.arange(1, n + 1, dtype=np.float32) / f(97.0)).astype(np.float32)
    lfo = g.binop(synth.K_MOD, g.binop(synth.K_MUL, synth.IN(0), synth.C(rates), n), synth.C(f(1.0)), n)
    amount = g.binop(synth.K_MUL, synth.C(f(depth)), lfo, n)
    return amount if base == 0.0 else g.binop(synth.K_SUM2, synth.C(f(base)), amount, n)


def _chorus(g, x, base=0.0, depth=CHORUS_DEPTH):
    """x + 0.5 * Delay(x, amount(t))."""
    n = len(x)
    wet = g.binop(synth.K_DELAY, x, _sweep(g, n, base, depth), n)
    return g.binop(synth.K_SUM2, x, g.binop(synth.K_MUL, synth.C(np.float32(0.5)), wet, n), n)


def _bus(g, V, P, seed=0x5EED0E10):
    """b = 0.5 * voice_0 + 0.25 * voice_1 + ... (the gains keep the matcher from folding the voices into one)."""
    v = D._voices(g, V, P, seed)
    bus = g.binop(synth.K_MUL, v[0:1], synth.C(np.float32(0.5)), 1)
    for k in range(1, V):
        bus = g.binop(synth.K_SUM2, bus, g.binop(synth.K_MUL, v[k:k + 1], synth.C(np.float32(0.5 ** (k + 1))), 1), 1)
    return bus


def env_fir_tree(V, P):
    """Row v: e = env * voice_v; y = e + 0.5 * Delay(e, 1): a two-tap low-pass behind an envelope."""
    g = synth.GraphArrays()
    return D._to_rows(g, _tap(g, _enveloped(g, V, P), 1, 0.5))


def env_taps_tree(V, P):
    """Row v: e = env * voice_v; y = e + Delay(e, 63); z = Delay(y, 1) + Delay(y, 64): three levels."""
    g = synth.GraphArrays()
    y = _tap(g, _enveloped(g, V, P), 63)
    z = g.binop(synth.K_SUM2, g.binop(synth.K_DELAY, y, synth.C(np.float32(1)), V), g.binop(synth.K_DELAY, y, synth.C(np.float32(64)), V), V)
    return D._to_rows(g, z)


def env_chorus_tree(V, P, base=0.0, depth=CHORUS_DEPTH):
    """Row v: e = env * voice_v; y = e + 0.5 * Delay(e, base + depth * Modulo(t * (v + 1) / 97, 1)): envelope, then chorus."""
    g = synth.GraphArrays()
    return D._to_rows(g, _chorus(g, _enveloped(g, V, P), base, depth))


def bus_chorus_tree(V, P, base=0.0, depth=CHORUS_DEPTH):
    """One row: b = sum of gain_v * voice_v; y = b + 0.5 * Delay(b, amount(t)): one chorus on the mix bus."""
    g = synth.GraphArrays()
    return D._to_rows(g, _chorus(g, _bus(g, V, P), base, depth))


def bus_fir_tree(V, P):
    """b; y = b + Delay(b, 7); z = y + Delay(y, 20); rows z, b: FIR stages behind a bus, and a row of a non-sink."""
    g = synth.GraphArrays()
    b = _bus(g, V, P)
    z = _tap(g, _tap(g, b, 7), 20)
    return D._to_rows(g, np.concatenate([z, b]))


def env_fir_gate_tree(V, P, d_in=30.0):
    """Row v: (e + 0.5 * Delay(e, 1)) + Delay(In(1), 30): env_fir next to a delayed control row (FR_STREAM_HISTORY next to
    FR_STREAM_TAPS).  A sum, not a product: the first 30 frames behind a seek, where the delayed row still reads 0.0, show the tap."""
    g = synth.GraphArrays()
    y = _tap(g, _enveloped(g, V, P), 1, 0.5)
    return D._to_rows(g, g.binop(synth.K_SUM2, y, np.broadcast_to(H._delayed_input(g, 1, d_in), (V,)), V))


def env_fir_beside_dry_tree(V, P, P_dry):
    """Rows 0 .. V-1: env_fir; row V: one dry voice of P_dry partials that writes its row: two banks (FR_STREAM_BANKS next to FR_STREAM_TAPS)."""
    g = synth.GraphArrays()
    y = _tap(g, _enveloped(g, V, P), 1, 0.5)
    return D._to_rows(g, np.concatenate([y, D._voices(g, 1, P_dry, 0x5EED0E20)]))


def chain_tree(V, P, levels):
    """Row v: x_0 = env * voice_v, x_k = x_(k-1) + 0.5 * Delay(x_(k-1), k): a chain of `levels` programs behind every voice
    (tools/stream_taps_probe.py: the slope over `levels` is the cost of one program hop).  levels == 1: the envelope alone."""
    g = synth.GraphArrays()
    x = _enveloped(g, V, P)
    for k in range(1, levels):
        x = _tap(g, x, k, 0.5)
    return D._to_rows(g, x)


def _case(name, build, n_rows, options, kernel, levels, short, dyn_ring=0, voices=2, per_voice=(), bus=0, segments=0, n_in=1, P=128, evals=2,
          knob=False, delay_rows=None, signal=None):
    """kernel: what the launch rule chooses; levels / short / dyn_ring: the three new keys; per_voice: programs_per_voice, sorted;
    evals: voice evaluations per frame of all rows together (the oracle's cost); delay_rows: the rows behind a constant Delay;
    signal: the case's builder with the signal amount's base raised by one frame (None: no signal delay)."""
    frames = min(STREAMS[0][0][1], H.G.ORACLE_LEAF_BUDGET // max(1, P * evals)) if voices else STREAMS[0][0][1]
    return {"name": name, "build": build, "n_rows": n_rows, "options": options, "kernel": kernel, "levels": levels, "short": short, "dyn_ring": dyn_ring,
            "voices": voices, "per_voice": sorted(per_voice), "bus": bus, "segments": segments, "n_in": n_in, "knob": knob, "semantics": "reference",
            "delay_rows": list(range(n_rows)) if delay_rows is None else list(delay_rows), "signal": signal, "oracle_frames": frames, "streams": STREAMS}


SERVABLE = [
    # level 1: e (one program per voice); level 2: y reads e at 0 and at 1
    _case("env_fir_2x128", lambda: env_fir_tree(2, 128), 2, OPTION, "bank_stream_prog_kernel", 2, 4, per_voice=[2, 2], evals=4),
    # e; y reads e at 0 and 63; z reads y at 1 (and at 64: an earlier block's)
    _case("env_taps_2x512", lambda: env_taps_tree(2, 512), 2, OPTION, "bank_stream_prog_kernel", 3, 6, per_voice=[3, 3], P=512, evals=8),
    # y reads e at 0 and by the signal amount
    _case("env_chorus_2x128", lambda: env_chorus_tree(2, 128), 2, DYN, "bank_stream_dyn_kernel", 2, 4, dyn_ring=2, per_voice=[2, 2], evals=4, delay_rows=(),
          signal=lambda: env_chorus_tree(2, 128, base=1.0)),
    # b reads three voices: a bus program; y reads b at 0 and by the signal amount: a bus program behind it
    _case("bus_chorus_3x128", lambda: bus_chorus_tree(3, 128), 1, BUS_DYN, "bank_stream_dyn_kernel", 2, 2, dyn_ring=1, voices=3, per_voice=[0, 0, 0], bus=2,
          evals=6, delay_rows=(), signal=lambda: bus_chorus_tree(3, 128, base=1.0)),
    # b (which writes row 1 itself and stores its ring), y (b at 0 and 7), z (y at 0 and 20): three bus programs
    _case("bus_fir_3x128", lambda: bus_fir_tree(3, 128), 2, BUS, "bank_stream_bus_kernel", 3, 4, voices=3, per_voice=[0, 0, 0], bus=3, evals=15, delay_rows=[0]),
    _case("fx_product_delay", F.product_delay_tree, 1, FX, "bank_stream_fx_kernel", 2, 1, voices=0, per_voice=[2], segments=1, n_in=3),
    _case("fx_product_knob_delay", F.product_knob_delay_tree, 1, FX_DYN, "bank_stream_fx_kernel", 2, 1, dyn_ring=1, voices=0, per_voice=[2], segments=1, n_in=4,
          knob=True, delay_rows=()),
    _case("general_env_fir_2x96", lambda: env_fir_tree(2, 96), 2, GENERAL, "bank_stream_general_kernel", 2, 4, per_voice=[2, 2], P=96, evals=4),
]

# FR_STREAM_TAPS next to the options no case above sets: the history's kernel and the bank table's take a level form as it is
COMPOSED = [
    _case("env_fir_gate_2x128", lambda: env_fir_gate_tree(2, 128), 2, dict(OPTION, FR_STREAM_INPUTS="1", FR_STREAM_HISTORY="1"), "bank_stream_hist_kernel", 2, 4,
          per_voice=[2, 2], n_in=2, evals=4),
    _case("env_fir_beside_dry", lambda: env_fir_beside_dry_tree(2, 128, 512), 3, dict(OPTION, FR_STREAM_BANKS="1"), "bank_stream_banks_kernel", 2, 4, voices=3,
          per_voice=[0, 2, 2], evals=8, delay_rows=[0, 1]),
]
ALL = SERVABLE + COMPOSED


def without(options, *keys):
    return {k: v for k, v in options.items() if k not in keys}


# (name, builder, output rows, options, input rows, the reason, word for word): what stays refused with FR_STREAM_TAPS on
REFUSED = [
    ("bus_fir_without_bus", lambda: bus_fir_tree(3, 128), 2, OPTION, 1, MIX_BUS),
    ("env_chorus_without_dyn", lambda: env_chorus_tree(2, 128), 2, OPTION, 1, D.OLD_REASON),
    # a feedback plan is untouched: a comb of 5 frames without FR_STREAM_LOOPS
    ("comb_5_with_taps", lambda: L.case("comb_5_2x128")["build"](), 2, OPTION, 1,
     "a program's ring is read 5 frames back; a streamed block needs delays of at least 64 frames"),
    # a bound observed from input rows
    ("observed_bound", lambda: D.observed_tree(2, 128), 2, dict(D.OBSERVED, FR_STREAM_TAPS="1"), 2,
     "a Delay's bound was observed from input rows (FR_DELAY_OBSERVED); a stream stores no rows, so block streaming does not serve it"),
]


def case(name):
    for c in ALL:
        if c["name"] == name:
            return c
    raise KeyError(name)


KNOB_SCALE = np.float32(36.0)                                   # control rows are within +-1.5: amounts within [0, 54)
KNOB_ABOVE = np.float32(60.0)                                   # beyond Minimum(., 48): the bound itself


def knob_amounts(row, idx):
    """fx_product_knob_delay's amount row (slot 3) in frames: |control| * 36 -- mostly inside (0, 48), fractional, some beyond the
    knob's 48 --, exactly 0 at every frame that is a multiple of 16 and 60 (the bound, after the Minimum) eight frames later."""
    with np.errstate(invalid="ignore", over="ignore"):
        a = (np.abs(row) * KNOB_SCALE).astype(np.float32)
    t = idx + np.arange(len(a))
    a[t % 16 == 0] = np.float32(0.0)
    a[t % 16 == 8] = KNOB_ABOVE
    return a


def streams_of(c, knob_raised=0.0):
    """The case's streams, [[(idx, T, rows)]]: stream_hist_cases.streams_of with the case's name as the control rows' seed; the knob of
    fx_product_knob_delay (slot 3) in frames (knob_amounts), `knob_raised` frames added to it."""
    streams = H.streams_of(dict(c, knob=False))
    if c["knob"]:
        streams = [[(idx, T, rows[:3] + [(knob_amounts(rows[3], idx) + np.float32(knob_raised)).astype(np.float32)]) for idx, T, rows in blocks] for blocks in streams]
    return streams


_REFERENCES = {}


def reference_of(name):
    """(tree, streams, expected blocks per stream) of a case: the dense reference, rendered once per process and left unchanged."""
    if name not in _REFERENCES:
        import stream_reference
        c = case(name)
        tree, streams = c["build"](), streams_of(c)
        _REFERENCES[name] = (tree, streams, [stream_reference.expected_blocks(tree, blocks, c["semantics"]) for blocks in streams])
    return _REFERENCES[name]


def frames_of(c):
    return sum(n for starts in c["streams"] for _, n in starts)


def check_stream_object(s, c, launched=False):
    """fr_plan_json["stream"] of a servable case against the graph's expectations.  `launched`: a resident launch has run (the prog
    and the bus kernel are named by the last launch, every later kernel of the cascade by the plan alone)."""
    assert s["servable"] is True and s["reason"] == "", s
    assert s["kernel"] == (c["kernel"] if launched or c["kernel"] not in NAMED_BY_LAUNCH else ""), s
    assert s["levels"] == c["levels"] and s["short_reads"] == c["short"] and s["dyn_ring_reads"] == c["dyn_ring"], s
    assert s["voices"] == c["voices"], s
    assert sorted(s["programs_per_voice"]) == c["per_voice"] and s["bus_programs"] == c["bus"], s
    assert s["input_slots"] == list(range(c["n_in"])), s
    if "segments" in s:
        assert s["segments"] == c["segments"], s
    else:
        assert c["segments"] == 0
    if "dyn_reads" in s:
        assert s["dyn_reads"] == c["dyn_ring"] and s["dyn_steps"] == 0 and s["lookback"] >= (CHORUS_DEPTH if c["signal"] else 0), s
    else:
        assert c["dyn_ring"] == 0


# ---- an edit inside a stream that stores its rows (tests/test_hip_stream_taps.py) ------------------------------------------------

STORE_DEPTH_AFTER = 35.0


def _depth_edges(tree):
    e = tree["edges"]
    at = np.nonzero((e[:, 0] == synth.CONST_HANDLE) & (e[:, 2] == int(np.float32(CHORUS_DEPTH).view(np.uint32))))[0]
    assert len(at) > 0
    return at


def with_depth(tree, depth=STORE_DEPTH_AFTER):
    """env_chorus's tree with the chorus depth constant -- the 70 of 70 * Modulo(...) -- set to `depth`."""
    e = tree["edges"].copy()
    e[_depth_edges(tree), 2] = int(np.float32(depth).view(np.uint32))
    return dict(tree, edges=e)


def edit_depth(r, tree, depth=STORE_DEPTH_AFTER):
    """The same edit on a renderer that has `tree` installed."""
    for i in _depth_edges(tree):
        _, node, bits, slot = (int(x) for x in tree["edges"][i])
        r.on_del_edge(synth.CONST_HANDLE, node, bits, slot)
        r.on_add_edge(synth.CONST_HANDLE, node, int(np.float32(depth).view(np.uint32)), slot)
