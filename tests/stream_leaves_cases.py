"""Patches for block streaming of COMPILED VOICES (FR_STREAM_LEAVES on top of FR_STREAM_PROGRAMS; csrc/leafprog.hpp,
csrc/streamplan.hpp), shared by the simulator tests (tests/test_stream_leaves_sim.py: the conditions on the inputs) and the GPU
tests of the two leaf kernels (tests/test_hip_stream_leaves.py).  Graph recipes and plain data: importable without a GPU.

A compiled voice is a balanced Sum2 tree over leaves of one expression shape that is not the hand-matched sine partial;
fr_fill_buffer renders it with a hipRTC-generated kernel, a stream interprets the leaf as a register program.  Each case is the
smallest shape at which a piece of the interpreter's walk can go wrong:
  tri_128        2 x 128 triangle partials      one chunk, one group of 8 per wave, the binary counter stops at level 3
  tri_chunks     2 x 512                        chunks of 128: stream_hand_over across 4 workgroups
  tri_carry1     M x 256                        M = the device's workgroups: one chunk of 256, two groups per wave
  tri_carry3     M x 1024                       8 groups per wave, carry levels 1..3 above the group
  tri_am         2 x 128, leaf x In(1)          a leaf that reads a control row (FR_STREAM_INPUTS); short and empty rows
  saw_div3       2 x 128, ((t w + ph) mod 1 - 0.5) / d     Divide, three varying columns
  literal_alias  a triangle voice with all amplitudes equal (a literal column) next to a voice whose two columns coincide
                 (an aliased column): two leaf banks (FR_STREAM_BANKS)
  tri_env_bus    a 128-partial triangle voice and a 128-partial template voice, an ADSR behind each, summed on a bus
                 (FR_STREAM_BANKS, FR_STREAM_BUS; both banks feed rings)
  tri_hostile    tri_128 on a time row of negative, NaN, +-inf, -0 and > 2^32 values, both semantics (exempt from the
                 finite-share condition)
`leaf_banks`: what fr_plan_json["stream"]["leaf_banks"] must say, from the graph: a triangle is 12 arithmetic ops in the tree form
(u = Modulo(t w, 1) - 0.5 stands twice) over 2 parameters (w, aliased; amp) and 1 input."""
import numpy as np

import stream_cases as K
import stream_input_cases as I
from libfriendship_amd import synth

KERNEL, STORE_KERNEL = "bank_stream_leaf_kernel", "bank_stream_leaf_store_kernel"
OPTION = dict(K.OPTION, FR_STREAM_LEAVES="1")                     # FR_STREAM_PROGRAMS + FR_STREAM_LEAVES
IDLE = {"FR_STREAM_IDLE_MS": "1500"}
OLD_REASON = "block streaming needs balanced template voices (these are general, compiled or track voices)"
OLD_REASON_PLAIN = "block streaming needs balanced template voices, one per output row"   # (without FR_STREAM_PROGRAMS' path)
FINITE_SHARE = 0.95
LOUD = 0.01
FRAMES, M_FRAMES = 1500, 300
SEED = 0x5EED0900
NEW_AMP = np.float32(0.5)                                          # the store case's edit: the third partial's amplitude, 1/3 -> 0.5


def _params(V, P, voices=None):
    p = synth.voice_params(V, P, SEED, wrap=48)
    w, amp = p["w"], p["amp"]
    if voices is not None:
        w, amp = w[np.asarray(voices)], amp[np.asarray(voices)]
    return w, amp


def _finish(g, roots):
    roots = np.asarray(roots, np.uint32).ravel()
    g.edge(roots, 0, 0, np.arange(len(roots), dtype=np.uint32))
    return g.finish(len(roots))


def tri_tree(V, P, am_slot=None, voices=None):
    """V voices x P triangle partials (synth.triangle_leaves), a row per voice; `voices`: only these (the same parameters)."""
    w, amp = _params(V, P, voices)
    g = synth.GraphArrays()
    return _finish(g, synth.sum_tree(g, synth.triangle_leaves(g, w, amp, 0, am_slot).reshape(w.shape)))


def saw_leaves(g, w, ph, d):
    """Divide(Sum2(Modulo(Sum2(t w, ph), 1), -0.5), d) per (w, ph, d)."""
    f = np.float32
    n = w.size
    x = g.binop(synth.K_SUM2, g.binop(synth.K_MUL, synth.IN(0), synth.C(w.ravel()), n), synth.C(ph.ravel()), n)
    u = g.binop(synth.K_SUM2, g.binop(synth.K_MOD, x, synth.C(f(1.0)), n), synth.C(f(-0.5)), n)
    return g.binop(synth.K_DIV, u, synth.C(d.ravel()), n)


def saw_tree(V, P):
    w, amp = _params(V, P)
    ph = (synth.uniform01(SEED + 1, V * P).reshape(V, P) - 0.3).astype(np.float32)      # offsets in (-0.3, 0.7]: the phase can go negative
    d = (np.float32(1.0) / amp).astype(np.float32)                                       # a divisor per partial: 1, 2, 3, ...
    g = synth.GraphArrays()
    return _finish(g, synth.sum_tree(g, saw_leaves(g, w, ph, d).reshape(V, P)))


def literal_alias_tree(P=128):
    """Row 0: a triangle voice whose amplitudes are all 1/16 (the column is a literal of the leaf program).  Row 1: the voice
    c * (Modulo(t c, 1) - 0.5) whose rate and gain are the same constant in every leaf (two columns coincide: one parameter)."""
    w, _ = _params(2, P)
    f = np.float32
    g = synth.GraphArrays()
    tri = synth.sum_tree(g, synth.triangle_leaves(g, w[0], np.full(P, f(0.0625)), 0).reshape(1, P))
    c = w[1].ravel()
    u = g.binop(synth.K_SUM2, g.binop(synth.K_MOD, g.binop(synth.K_MUL, synth.IN(0), synth.C(c), P), synth.C(f(1.0)), P), synth.C(f(-0.5)), P)
    saw = synth.sum_tree(g, g.binop(synth.K_MUL, synth.C(c), u, P).reshape(1, P))
    return _finish(g, [tri[0], saw[0]])


def env_bus_tree(P=128):
    """One row: ADSR x a triangle voice + ADSR x a template voice.  The tree carries the triangle leaves' handles and amplitudes
    for the store test's edit."""
    w, amp = _params(2, P)
    g = synth.GraphArrays()
    leaves = synth.triangle_leaves(g, w[0], amp[0], 0)
    tri = synth.sum_tree(g, leaves.reshape(1, P))
    sine = synth.sum_tree(g, synth.partial_leaves(g, w[1], amp[1], 0).reshape(1, P))
    env = synth.adsr_envelope(g)
    x = g.binop(synth.K_MUL, np.broadcast_to(env, (2,)), np.array([tri[0], sine[0]], np.uint32), 2)
    t = _finish(g, [g.binop(synth.K_SUM2, x[0:1], x[1:2], 1)[0]])
    t["tri_leaves"], t["tri_amp"] = leaves, amp[0].copy()
    return t


def edit_amplitude(r, tree):
    """The third triangle partial's amplitude from 1/3 to NEW_AMP: the compiled bank's parameter table changes."""
    leaf, old = int(tree["tri_leaves"][2]), tree["tri_amp"][2]
    r.on_del_edge(synth.CONST_HANDLE, leaf, int(synth.bits(old)), 0)
    r.on_add_edge(synth.CONST_HANDLE, leaf, int(synth.bits(NEW_AMP)), 0)


def leaf33_tree(V=2, P=128):
    """A triangle partial and 21 more additions of 2^-20: 33 arithmetic ops, one over the interpreter's limit."""
    w, amp = _params(V, P)
    g = synth.GraphArrays()
    x = synth.triangle_leaves(g, w, amp, 0)
    for _ in range(21):
        x = g.binop(synth.K_SUM2, x, synth.C(np.float32(2.0 ** -20)), V * P)
    return _finish(g, synth.sum_tree(g, x.reshape(V, P)))


def tri_flanger_tree(V=2, P=128, base=8.0, depth=6.0, rate=0.01, gain=0.5):
    """synth.feedback_flanger over triangle voices: a sweep plan (FR_LOOP_DYN) behind a compiled bank."""
    w, amp = _params(V, P)
    g = synth.GraphArrays()
    f = np.float32
    voice = synth.sum_tree(g, synth.triangle_leaves(g, w, amp, 0).reshape(V, P))
    rates = (f(rate) * np.arange(1, V + 1, dtype=np.float32)).astype(np.float32)
    ramp = g.binop(synth.K_MOD, g.binop(synth.K_MUL, synth.IN(0), synth.C(rates), V), synth.C(f(1.0)), V)
    amount = g.binop(synth.K_SUM2, synth.C(f(base)), g.binop(synth.K_MUL, synth.C(f(depth)), g.binop(synth.K_MIN, synth.C(f(1.0)), ramp, V), V), V)
    x = g.nodes(synth.K_SUM2, V)
    wet = g.binop(synth.K_DELAY, x, amount, V)
    g.edge(voice, x, 0, 0)
    g.edge(g.binop(synth.K_MUL, wet, synth.C(f(gain)), V), x, 0, 1)
    return _finish(g, x)


# (name, build, output rows, options, declared track slots from, the sentence): refused with the feature on, each with its own sentence
STILL_REFUSED = [
    ("tri_64", lambda: tri_tree(2, 64), 2, OPTION, None,
     "compiled voices of 64 partials; block streaming interprets the leaves of voices of at least 128 partials (16 waves x one group of 8)"),
    ("track_voice", lambda: synth.track_tree(2, 128), 2, dict(OPTION, FR_STREAM_INPUTS="1"), 1,
     "these compiled voices read per-leaf track rows (track voices); block streaming interprets leaves over constants and streamed input rows only"),
    ("leaf_33_ops", leaf33_tree, 2, OPTION, None, "a leaf of 33 arithmetic ops; block streaming interprets leaves of at most 32"),
    ("sweep_plan", tri_flanger_tree, 2, dict(OPTION, FR_LOOP_DYN="1", FR_STREAM_LOOPS="1", FR_STREAM_DYN="1", FR_STREAM_SWEEP="1"), None,
     "a sweep plan (a feedback loop that delays by a signal amount) together with compiled voices; block streaming has no sweep form with a leaf interpreter"),
]

TRI = {"ops": 12, "params": 2, "inputs": 1}


class Case:
    """`build(M)`: the tree (M = stream.max_workgroups; only the M-voice cases use it); `rows(M)`: its output rows; `sample`: the
    voices the oracle renders of an M-voice case (a patch of those voices alone, same parameters) and `oracle` its frames."""

    def __init__(self, name, build, rows, options=OPTION, n_in=1, leaf_banks=(TRI,), frames=FRAMES, oracle=FRAMES, sample=None, oracle_build=None,
                 hostile=False, banks=1):
        self.name, self.build, self.rows, self.options, self.n_in = name, build, rows, dict(options), n_in
        self.leaf_banks, self.frames, self.oracle, self.sample, self.oracle_build = list(leaf_banks), frames, oracle, sample, oracle_build
        self.hostile, self.banks = hostile, banks

    def n_rows(self, M=0):
        return self.rows(M) if callable(self.rows) else self.rows


def _m_case(name, P, oracle):
    sample = lambda M: [0, M - 1]
    return Case(name, lambda M: tri_tree(M, P), lambda M: M, frames=M_FRAMES, oracle=oracle, sample=sample,
                oracle_build=lambda M: tri_tree(M, P, voices=sample(M)))


CASES = [
    Case("tri_128", lambda M=0: tri_tree(2, 128), 2),
    Case("tri_chunks", lambda M=0: tri_tree(2, 512), 2),
    _m_case("tri_carry1", 256, M_FRAMES),
    _m_case("tri_carry3", 1024, 96),
    Case("tri_am", lambda M=0: tri_tree(2, 128, am_slot=1), 2, options=dict(OPTION, FR_STREAM_INPUTS="1"), n_in=2,
         leaf_banks=[{"ops": 13, "params": 2, "inputs": 2}]),
    Case("saw_div3", lambda M=0: saw_tree(2, 128), 2, leaf_banks=[{"ops": 5, "params": 3, "inputs": 1}]),
    Case("literal_alias", lambda M=0: literal_alias_tree(), 2, options=dict(OPTION, FR_STREAM_BANKS="1"),
         leaf_banks=[{"ops": 12, "params": 1, "inputs": 1}, {"ops": 4, "params": 1, "inputs": 1}], banks=2),
    Case("tri_env_bus", lambda M=0: env_bus_tree(), 1, options=dict(OPTION, FR_STREAM_BANKS="1", FR_STREAM_BUS="1"), banks=2),
    Case("tri_hostile", lambda M=0: tri_tree(2, 128), 2, hostile=True),
]
IDS = [c.name for c in CASES]
SIM_M = 4                                                          # the M-voice cases on the simulator: the conditions do not depend on M


def case(name):
    for c in CASES:
        if c.name == name:
            return c
    raise KeyError(name)


HOSTILE_TIMES = np.array([-1.0, -0.0, 0.0, -48000.25, np.nan, np.inf, -np.inf, 4294967296.0, 4294967808.0, 1e30, -1e30, 1e-42, -1e-42, 16777216.0, 0.5], np.float32)


def blocks_of(c, starts, seed=53):
    """[(idx, T, rows)]: stream_cases.finite_block_rows' blocks (the first seven of fixed lengths, then 1..64; special finite times on
    every fifth block, +-inf and NaN on a segment's last).  tri_am: a control row of every kind but the hostile one -- full, short
    (padded with its last value), empty (missing: the slot goes on with its last value), constant, ramp; a slot that was fed
    cannot be left out of a later block, in a stream as in fr_fill_buffer.  tri_hostile: HOSTILE_TIMES over half of every row."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (idx, t) in enumerate(K.finite_block_rows(rng, starts)):
        T = len(t)
        rows = [np.array(t, np.float32)]
        if c.hostile:
            at = rng.permutation(T)[:(T + 1) // 2]
            rows[0][at] = HOSTILE_TIMES[rng.integers(len(HOSTILE_TIMES), size=len(at))]
        if c.n_in == 2:
            rows.append(I.control_row(rng, T, k % 5 if k else 0))
        out.append((idx, T, rows))
    return out


def short_blocks_of(c):
    """Blocks of 64, 1 and 37 frames from frame 0."""
    return [(idx, len(t), [t]) for idx, t in K.short_blocks(0)]


def condition_message(name, exp):
    """'' when every row of `exp` is at least FINITE_SHARE finite and louder than LOUD somewhere."""
    for r, row in enumerate(np.asarray(exp)):
        fin = np.isfinite(row)
        if fin.mean() < FINITE_SHARE:
            return f"{name}: row {r} is {fin.mean():.3f} finite, below {FINITE_SHARE}"
        if not (np.abs(row[fin]).max() > LOUD):
            return f"{name}: row {r} never exceeds {LOUD}"
    return ""


def fill_blocks(lib, tree, n_rows, blocks, semantics="reference", edit_before=None, options=None, upto=None):
    """The blocks through fr_fill_buffer of a renderer of `lib` without a stream option (on the HIP library: the compiled kernel).
    `edit_before`: the block before which edit_amplitude is applied; `upto`: only the frames before that one."""
    from libfriendship_amd.capi import Renderer
    out = []
    with Renderer(lib, semantics=semantics, options=dict(options) if options else None) as f:   # (the oracle takes no options)
        synth.install(f, tree)
        for k, (idx, T, rows) in enumerate(blocks):
            if upto is not None:
                T = min(T, upto - idx)
                if T <= 0:
                    break
            if edit_before is not None and k == edit_before:
                edit_amplitude(f, tree)
            out.append(f.fill_buffer(n_rows, idx, idx + T, [r[:T] for r in rows]))
    return out


def stream_blocks(lib, tree, n_rows, blocks, options, semantics="reference", edit_before=None):
    """The blocks through fr_stream_block_rows of one renderer; `edit_before`: the block before which the stream is closed, the
    amplitude edited and a stream begun again (a store stream continues at the renderer's head).  Returns the blocks' results and
    the "stream" objects read after the first block and at the end."""
    from libfriendship_amd.capi import Renderer
    with Renderer(lib, semantics=semantics, options=dict(options, **IDLE)) as s:
        synth.install(s, tree)
        s.stream_begin(n_rows)
        got, first = [], None
        for k, (idx, T, rows) in enumerate(blocks):
            if edit_before is not None and k == edit_before:
                s.stream_end()
                edit_amplitude(s, tree)
                s.stream_begin(n_rows)
            got.append(s.stream_block_rows(idx, rows, n_times=T))
            if k == 0:
                first = s.plan()["stream"]
        last = s.plan()["stream"]
        s.stream_end()
    return got, first, last


def compare_blocks(got, exp, blocks, what, rows=None):
    """Every sample of every block equal bit for bit (NaN = NaN, +0 != -0); `rows`: only these rows of `got` (against all of
    `exp`); `exp` may stop early (an oracle prefix).  Returns the frames compared."""
    n = 0
    for k, ((idx, T, _), a, b) in enumerate(zip(blocks, got, exp)):
        a = a if rows is None else a[np.asarray(rows)]
        a = a[:, :b.shape[1]]
        assert K.same_bits(a, b), f"{what}: block {k} at frame {idx} (T={T}): " + K.first_diff(a, b)
        n += b.shape[1]
    return n


def check_stream_object(s, c, M=0, store=False):
    """fr_plan_json["stream"] of a served case against the graph's expectations."""
    assert s["servable"] is True and s["reason"] == "", (c.name, s)
    assert s["kernel"] == (STORE_KERNEL if store else KERNEL), (c.name, s)
    assert [{k: b[k] for k in ("ops", "params", "inputs")} for b in s["leaf_banks"]] == c.leaf_banks, (c.name, s)
    assert all(1 <= b["regs"] <= 8 for b in s["leaf_banks"]), (c.name, s)
    assert s["input_slots"] == list(range(c.n_in)), (c.name, s)
    assert s["voices"] == (c.n_rows(M) if c.name != "tri_env_bus" else 2), (c.name, s)
