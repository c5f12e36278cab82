"""Patches for block streaming of TRACK VOICES (FR_STREAM_TRACKS on top of FR_STREAM_PROGRAMS and FR_STREAM_LEAVES;
csrc/leafprog.hpp, csrc/streamplan.hpp), shared by the simulator tests (tests/test_stream_tracks_sim.py: the conditions on the
inputs) and the GPU tests of the two track kernels (tests/test_hip_stream_tracks.py).  Graph recipes and plain data: importable
without a GPU.

A track voice is a balanced Sum2 tree over synth.track_leaves: every partial's phase increment w and amplitude are read per frame
from its own pair of input rows (fr_set_track_inputs).  A block brings them as a dense matrix [first_track + 2 V P, T]
(fr_stream_block_dense), the twin takes the same matrix through fr_fill_buffer_dense.  Each case is the smallest shape at which
a piece of the walk can go wrong:
  trk_128        2 x 128                         one chunk, one group of 8 per wave: the one-ahead loads run 7 times per wave
  trk_chunks     2 x 512                         chunks of 128 over 4 workgroups each: stream_hand_over
  trk_carry      M x 256, w a track, amp a constant     M = the device's workgroups: one chunk of 256, two groups per wave, carry
                 level 1.  ONE track per partial: with two, a patch whose chunks are larger than 128 partials on a whole device
                 names more than 2 x 128 x 256 = 65536 rows, which is the staging's limit -- the carry chain above a group is
                 reachable with tracks only for such a leaf (or on a partitioned device)
  trk_cap        M x 128                         at M = 256 exactly 65536 staged rows
  trk_am         2 x 128, leaf x In(1)           a track leaf that also reads a control row (FR_STREAM_INPUTS; tracks from slot 2);
                 every third block goes through fr_stream_block_rows with a short or empty control row and no matrix: its tracks
                 read +0.0
  trk_env_bus    row 0: a 128-partial track voice; row 1: two 128-partial template voices, an ADSR behind each, summed on a bus
                 (FR_STREAM_BANKS, FR_STREAM_BUS): a track bank next to a bank with programs and a bus segment in one launch.
                 The track voice itself writes its row: a track voice that feeds a delay line or a program is refused by the
                 planner for every entry point (stage.cpp check_tracks: tracks are never stored) unless FR_TRACK_HISTORY is on,
                 which a stream refuses -- so no envelope can stand behind the track voice, in a stream or in its twin
  trk_unprimed   trk_128 without the priming call: the slot limit of the first block, 2 x 64 = 128, is the amp slot of partial 63
                 of voice 0 -- its w row is read, its amp row is not
  trk_short      trk_128 with matrices of 1 + 2 x 100 + 1 rows: n_in_rows is the limit, between a w and an amp slot
  trk_hostile    trk_128 with tests/track_rows.py's hostile w and amp values in the first and last group of voice 0 and the whole
                 share of wave 1 of voice 1, at frames 0, 63 and T - 1 of every block, on a hostile time row; both semantics
The expected rows of the synth.track_tree cases are bank_reference.render_track_bank's on every frame, under the slot limit the
reference keeps (track_rows.SlotLimit)."""
import numpy as np

import bank_reference
import stream_cases as K
import stream_input_cases as I
import track_rows as TR
from libfriendship_amd import synth

KERNEL, STORE_KERNEL = "bank_stream_track_kernel", "bank_stream_track_store_kernel"
OPTION = dict(K.OPTION, FR_STREAM_LEAVES="1", FR_STREAM_TRACKS="1")
IDLE = {"FR_STREAM_IDLE_MS": "1500"}
OLD_REASON = "these compiled voices read per-leaf track rows (track voices); block streaming interprets leaves over constants and streamed input rows only"
HISTORY_REASON = "block streaming with a track history"
FINITE_SHARE = 0.95
LOUD = 0.01
FRAMES, M_FRAMES = 1500, 300
SEED = 0x5EED0A00
LIMIT = 65536
_F = np.float32


def _finish(g, roots):
    roots = np.asarray(roots, np.uint32).ravel()
    g.edge(roots, 0, 0, np.arange(len(roots), dtype=np.uint32))
    return g.finish(len(roots))


def track_tree(V, P, first=1, am_slot=None, voices=None):
    """synth.track_tree's voices (slot first + 2 (v P + k) holds w, the next one amp), a row per voice; `am_slot`: every leaf
    times that input; `voices`: only these, with the slots they have in the whole patch."""
    vs = np.arange(V) if voices is None else np.asarray(voices)
    g = synth.GraphArrays()
    w_slots = (first + 2 * (vs[:, None] * P + np.arange(P)[None, :])).astype(np.uint32).ravel()
    leaves = synth.track_leaves(g, w_slots, w_slots + 1)
    if am_slot is not None:
        leaves = g.binop(synth.K_MUL, leaves, synth.IN(am_slot), len(w_slots))
    return _finish(g, synth.sum_tree(g, leaves.reshape(len(vs), P)))


def carry_amp(V, P):
    return (np.tile(_F(1.0) / np.arange(1, P + 1, dtype=_F), (V, 1)) * (_F(1.0) + _F(0.001) * np.arange(V, dtype=_F)[:, None])).astype(_F)


def w_track_tree(V, P, first=1, voices=None):
    """The partial whose w is a track (slot first + v P + k) and whose amplitude is a constant: one track per partial."""
    vs = np.arange(V) if voices is None else np.asarray(voices)
    amp = carry_amp(V, P)[vs]
    n = len(vs) * P
    g = synth.GraphArrays()
    f = _F
    x = g.nodes(synth.K_MUL, n)
    g.edge(0, x, 0, 0)
    g.edge(0, x, (first + vs[:, None] * P + np.arange(P)[None, :]).astype(np.uint32).ravel(), 1)
    ph = g.binop(synth.K_MOD, x, synth.C(f(1.0)), n)
    u = g.binop(synth.K_SUM2, ph, synth.C(f(-0.5)), n)
    m = g.binop(synth.K_MIN, u, g.binop(synth.K_MUL, synth.C(f(-1.0)), u, n), n)
    n1 = g.binop(synth.K_MUL, synth.C(f(-1.0)), g.binop(synth.K_MUL, synth.C(f(-1.0)), m, n), n)
    q = g.binop(synth.K_SUM2, synth.C(f(0.5)), n1, n)
    y = g.binop(synth.K_MUL, g.binop(synth.K_MUL, synth.C(f(-16.0)), u, n), q, n)
    return _finish(g, synth.sum_tree(g, g.binop(synth.K_MUL, synth.C(amp.ravel()), y, n).reshape(len(vs), P)))


def env_bus_tree(P=128):
    """Row 0: a track voice.  Row 1: ADSR x a template voice + ADSR x a second template voice.  The tree carries the first template
    voice's leaves' handles and amplitudes for the store test's edit."""
    p = synth.voice_params(2, P, SEED, wrap=48)
    g = synth.GraphArrays()
    w_slots = (1 + 2 * np.arange(P)).astype(np.uint32)
    trk = synth.sum_tree(g, synth.track_leaves(g, w_slots, w_slots + 1).reshape(1, P))
    leaves = synth.partial_leaves(g, p["w"], p["amp"], 0)
    sine = synth.sum_tree(g, leaves.reshape(2, P))
    env = synth.adsr_envelope(g)
    x = g.binop(synth.K_MUL, np.broadcast_to(env, (2,)), sine, 2)
    t = _finish(g, [trk[0], g.binop(synth.K_SUM2, x[0:1], x[1:2], 1)[0]])
    t["sine_leaves"], t["sine_amp"] = leaves, p["amp"][0].copy()
    return t


NEW_AMP = _F(0.75)                                                    # the store case's edit: the third template partial's amplitude, 1/3 -> 0.75


def edit_amplitude(r, tree):
    leaf, old = int(tree["sine_leaves"][2]), tree["sine_amp"][2]
    r.on_del_edge(synth.CONST_HANDLE, leaf, int(synth.bits(old)), 0)
    r.on_add_edge(synth.CONST_HANDLE, leaf, int(synth.bits(NEW_AMP)), 0)


class Case:
    """`V(M)`, `P`: the track bank's voices and partials (M = stream.max_workgroups); `build(M, voices)`: the tree, or the patch of
    those voices alone for the oracle; `tracks`: rows per partial (2: w and amp; 1: w); `first`: the first track slot; `dense`: the
    expected rows are render_track_bank's."""

    def __init__(self, name, V, P, build, options=OPTION, first=1, tracks=2, frames=FRAMES, oracle=FRAMES, sample=None, dense=True, rows=None, prime=True,
                 short=None, hostile=False, banks=1, ops=11, params=2, exempt=()):
        self.name, self._V, self.P, self.build, self.options = name, V, P, build, dict(options)
        self.first, self.tracks, self.frames, self.oracle, self.sample, self.dense = first, tracks, frames, oracle, sample, dense
        self.exempt = tuple(exempt)                                  # rows outside the finite-and-audible condition, each for a stated reason
        self._rows, self.prime, self.short, self.hostile, self.banks, self.ops, self.params = rows, prime, short, hostile, banks, ops, params

    def V(self, M=0):
        return self._V(M) if callable(self._V) else self._V

    def n_rows(self, M=0):
        return self._rows if self._rows is not None else self.V(M)

    def n_in(self, M=0):
        """Rows of a block's whole matrix."""
        return self.first + self.tracks * self.V(M) * self.P

    def staged(self, M=0):
        return self.tracks * self.V(M) * self.P


_two = lambda M=0, voices=None: track_tree(2, 128, voices=voices)
CASES = [
    Case("trk_128", 2, 128, _two),
    Case("trk_chunks", 2, 512, lambda M=0, voices=None: track_tree(2, 512, voices=voices)),
    Case("trk_carry", lambda M: M, 256, lambda M, voices=None: w_track_tree(M, 256, voices=voices), tracks=1, frames=M_FRAMES, oracle=96, sample=lambda M: [0, M - 1]),
    Case("trk_cap", lambda M: M, 128, lambda M, voices=None: track_tree(M, 128, voices=voices), frames=M_FRAMES, oracle=96, sample=lambda M: [0, M - 1]),
    Case("trk_am", 2, 128, lambda M=0, voices=None: track_tree(2, 128, first=2, am_slot=1, voices=voices), options=dict(OPTION, FR_STREAM_INPUTS="1"), first=2, dense=False, ops=12),
    Case("trk_env_bus", 1, 128, lambda M=0, voices=None: env_bus_tree(), options=dict(OPTION, FR_STREAM_BANKS="1", FR_STREAM_BUS="1"), dense=False, rows=2, banks=2),
    Case("trk_unprimed", 2, 128, _two, prime=False, exempt=(1,)),    # (voice 1's slots all lie beyond the limit 128 for good: it is +0.0, which is the point)
    Case("trk_short", 2, 128, _two, short=1 + 2 * 100 + 1, exempt=(1,)),   # (voice 1's rows are never handed in: +0.0)
    Case("trk_hostile", 2, 128, _two, hostile=True, exempt=(0, 1)),
]
IDS = [c.name for c in CASES]
SIM_M = 4                                                              # the M-voice cases on the CPU: a voice's row does not depend on how many there are


def case(name):
    for c in CASES:
        if c.name == name:
            return c
    raise KeyError(name)


def matrix(c, M, idx, t, k, rng):
    """The dense matrix of block k at frame idx with the time row t: track rows random per element (a read of another frame,
    partial or block gets other values): small positive w, amplitudes 1/(k+1) scaled by 0.5 .. 1.5."""
    V, P, T = c.V(M), c.P, len(t)
    n = V * P
    m = np.zeros((c.n_in(M), T), _F)
    m[0] = t
    w = rng.random((n, T), dtype=_F) * _F(0.05)
    if c.tracks == 1:
        m[c.first:] = w
    else:
        m[c.first::2] = w
        m[c.first + 1::2] = (rng.random((n, T), dtype=_F) + _F(0.5)) * np.tile(_F(1.0) / np.arange(1, P + 1, dtype=_F), V)[:, None]
    if c.first == 2:
        m[1] = I.control_row(rng, T, 4 if k % 5 == 4 else 0)          # full rows: constant or a ramp of every kind but the hostile one
        if len(m[1]) != T:
            raise AssertionError("a dense block's control row is full length")
    if c.hostile:
        m[0] = TR.HOSTILE_ODD[(np.arange(T) + k) % len(TR.HOSTILE_ODD)] if k % 4 == 3 else t
        at = rng.permutation(T)[:T // 3]
        m[0, at] = np.concatenate([TR.HOSTILE_NEG, TR.HOSTILE_ODD])[rng.integers(24, size=len(at))]
        for v, k0, cnt in ((0, 0, 8), (0, P - 8, 8), (1, P // 16, P // 16)):   # the first and last group of voice 0, wave 1's share of voice 1
            for j in range(k0, k0 + cnt):
                slot = c.first + 2 * (v * P + j)
                for q, f in enumerate(sorted({0, 63, T - 1} & set(range(T)))):
                    m[slot, f] = TR.HOSTILE_W[(j + 3 * q + k) % len(TR.HOSTILE_W)]
                    m[slot + 1, f] = TR.HOSTILE_AMP[(5 * j + q + k) % len(TR.HOSTILE_AMP)]
    if c.short is not None:
        m = np.ascontiguousarray(m[:c.short])
    return m


def blocks_of(c, M, starts, seed=61):
    """[(idx, T, matrix, rows)]: stream_cases.finite_block_rows' blocks (the first seven of fixed lengths, then 1..64).  `rows`
    is None for a dense block; trk_am: every third block is a rows-only block -- [time row, control row] with a short or an
    empty control row, through fr_stream_block_rows and fr_fill_buffer."""
    rng = np.random.default_rng([seed, c.V(M), c.P])
    out = []
    for k, (idx, t) in enumerate(K.finite_block_rows(rng, starts)):
        m = matrix(c, M, idx, np.array(t, _F), k, rng)
        rows = None
        if c.first == 2 and k % 3 == 2:
            T = len(t)
            rows = [m[0].copy(), m[1][:0] if k % 2 else m[1][:(T + 1) // 2].copy()]
        out.append((idx, len(t), m, rows))
    return out


def short_blocks_of(c, M=0):
    rng = np.random.default_rng(67)
    return [(idx, len(t), matrix(c, M, idx, np.array(t, _F), k, rng), None) for k, (idx, t) in enumerate(K.short_blocks(0))]


def priming(c, M):
    """(n_slots, matrix) of the call that makes every row live: n_slots * 64 >= the matrix's rows."""
    rng = np.random.default_rng(71)
    n_slots = max(c.n_rows(M), -(-c.n_in(M) // 64))
    return n_slots, matrix(c, M, 0, synth.time_ramp(0, 64), 0, rng)


def expected_dense(c, M, blocks, voices=None):
    """bank_reference.render_track_bank over the blocks under the reference's slot limit (the priming call included); `voices`:
    only these rows."""
    V, P = c.V(M), c.P
    limit = TR.SlotLimit()
    if c.prime:
        limit.call(priming(c, M)[0], 64)
    out = []
    for idx, T, m, rows in blocks:
        lim = min(limit.call(c.n_rows(M), T), m.shape[0]) if rows is None else 0
        if c.tracks == 2:
            w, amp = bank_reference.track_params(m, V, P, lim, first_track=c.first)
        else:
            w = np.zeros((V * P, T), _F)
            have = max(0, min(lim - c.first, V * P))
            w[:have] = m[c.first:c.first + have]
            w = w.reshape(V, P, T)
            amp = np.broadcast_to(carry_amp(V, P)[:, :, None], w.shape)
        if voices is not None:
            w, amp = w[np.asarray(voices)], np.asarray(amp)[np.asarray(voices)]
        out.append(bank_reference.render_track_bank(w, amp, m[0]))
    return out


def condition_message(name, exp, skip=()):
    """'' when every row of `exp` outside `skip` is at least FINITE_SHARE finite and louder than LOUD somewhere."""
    for r, row in enumerate(np.asarray(exp)):
        if r in skip:
            continue
        fin = np.isfinite(row)
        if fin.mean() < FINITE_SHARE:
            return f"{name}: row {r} is {fin.mean():.3f} finite, below {FINITE_SHARE}"
        if not (np.abs(row[fin]).max() > LOUD):
            return f"{name}: row {r} never exceeds {LOUD}"
    return ""


def rows_differ_message(name, blocks):
    """'' when consecutive dense blocks' matrices differ in every row over the frames they share (a stale read would show)."""
    dense = [b for b in blocks if b[3] is None]
    for (_, Ta, a, _), (idx, Tb, b, _) in zip(dense, dense[1:]):
        n = min(Ta, Tb)
        same = np.all(a[:, :n].view(np.uint32) == b[:, :n].view(np.uint32), axis=1) if a.shape[0] == b.shape[0] else np.array([True])
        if same.any():
            return f"{name}: the block at frame {idx} repeats row {int(np.argmax(same))} of the block before"
    return ""


def fill_blocks(lib, c, M, blocks, semantics="reference", tree=None, n_rows=None, edit_before=None, options=None, upto=None, csr=False):
    """The blocks through fr_fill_buffer_dense of a renderer of `lib` without a stream option (on the HIP library: the generated
    jit_bank kernel with tracks) after the priming call; rows-only blocks through fr_fill_buffer.  `csr`: every block through
    fr_fill_buffer with its rows as a list (the oracle, which has no dense entry); `upto`: only the frames before that one."""
    from libfriendship_amd.capi import Renderer
    tree = c.build(M) if tree is None else tree
    n_rows = c.n_rows(M) if n_rows is None else n_rows
    out = []
    with Renderer(lib, semantics=semantics, options=dict(options) if options else None) as f:
        if not csr:
            f.set_track_inputs(c.first)
        synth.install(f, tree)
        if c.prime:
            n_slots, m0 = priming(c, M)
            f.fill_buffer(n_slots, 0, 64, list(m0)) if csr else f.fill_buffer_dense(n_slots, 0, 64, m0)
        for k, (idx, T, m, rows) in enumerate(blocks):
            if upto is not None:
                T = min(T, upto - idx)
                if T <= 0:
                    break
            if edit_before is not None and k == edit_before:
                edit_amplitude(f, tree)
            if rows is not None:                                      # (the oracle stores every slot: its track slots go on, with the +0.0 they read)
                zeros = [np.zeros(T, _F)] * (m.shape[0] - len(rows)) if csr else []
                out.append(f.fill_buffer(n_rows, idx, idx + T, [r[:T] for r in rows] + zeros))
            elif csr:
                out.append(f.fill_buffer(n_rows, idx, idx + T, list(m[:, :T])))
            else:
                out.append(f.fill_buffer_dense(n_rows, idx, idx + T, np.ascontiguousarray(m[:, :T])))
    return out


def stream_blocks(lib, c, M, blocks, options=None, semantics="reference", edit_before=None, tree=None):
    """The blocks through fr_stream_block_dense (rows-only blocks: fr_stream_block_rows) of one renderer after the priming call;
    `edit_before`: the block before which the stream is closed, the amplitude edited and a stream begun again.  Returns the
    blocks' results and the "stream" objects read after the first block and at the end."""
    from libfriendship_amd.capi import Renderer
    tree = c.build(M) if tree is None else tree
    n_rows = c.n_rows(M)
    with Renderer(lib, semantics=semantics, options=dict(c.options if options is None else options, **IDLE)) as s:
        s.set_track_inputs(c.first)
        synth.install(s, tree)
        if c.prime:
            n_slots, m0 = priming(c, M)
            s.fill_buffer_dense(n_slots, 0, 64, m0)
        s.stream_begin(n_rows)
        got, first = [], None
        for k, (idx, T, m, rows) in enumerate(blocks):
            if edit_before is not None and k == edit_before:
                s.stream_end()
                edit_amplitude(s, tree)
                s.stream_begin(n_rows)
            got.append(s.stream_block_dense(idx, m) if rows is None else s.stream_block_rows(idx, rows, n_times=T))
            if k == 0:
                first = s.plan()["stream"]
        last = s.plan()["stream"]
        s.stream_end()
    return got, first, last


def compare_blocks(got, exp, blocks, what, rows=None):
    """Every sample of every block equal bit for bit (NaN = NaN, +0 != -0); `rows`: only these rows of `got` (against all of
    `exp`); `exp` may stop early (an oracle prefix).  Returns the frames compared."""
    n = 0
    for k, ((idx, T, _, _), a, b) in enumerate(zip(blocks, got, exp)):
        a = a if rows is None else a[np.asarray(rows)]
        a = a[:, :b.shape[1]]
        assert K.same_bits(a, b), f"{what}: block {k} at frame {idx} (T={T}): " + K.first_diff(a, b)
        n += b.shape[1]
    return n


def check_stream_object(s, c, M=0, store=False):
    """fr_plan_json["stream"] of a served case against the graph's expectations."""
    assert s["servable"] is True and s["reason"] == "", (c.name, s)
    assert s["kernel"] == (STORE_KERNEL if store else KERNEL), (c.name, s)
    assert s["tracks"] == {"first_slot": c.first, "rows": c.staged(M), "limit": LIMIT}, (c.name, s["tracks"])
    assert len(s["leaf_banks"]) == 1 and s["leaf_banks"][0]["track_cols"] == c.tracks and s["leaf_banks"][0]["params"] == c.params, (c.name, s["leaf_banks"])
    assert 11 <= s["leaf_banks"][0]["ops"] <= 32 and 1 <= s["leaf_banks"][0]["regs"] <= 8, (c.name, s["leaf_banks"])
    assert s["input_slots"] == list(range(c.first)), (c.name, s)
    assert s["voices"] == (c.V(M) if c.banks == 1 else 3), (c.name, s)
