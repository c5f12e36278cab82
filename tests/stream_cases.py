"""Patches for block streaming of plans with programs (FR_STREAM_PROGRAMS), shared by the simulator tests of the serving rule
(tests/test_stream_plan_sim.py) and the GPU tests of the resident kernel (tests/test_hip_stream_programs.py).

A case is (name, tree builder, voices, expectation).  For a servable case the expectation is the number of programs the rule
must deal to every voice, derived from the graph:
  * a feed-forward patch (envelope and / or taps behind each voice) has ONE program per voice in its one-launch form: the
    voice's output row, with the chain's intermediate taps stored to their rings on the way;
  * a comb x = voice + g * Delay(x, d) is one loop per voice: one program per voice that stores the loop's ring and writes
    the row.
For a refused case it is a fragment of the reason fr_plan_json and fr_last_error must give."""
import numpy as np

from libfriendship_amd import synth

OPTION = {"FR_STREAM_PROGRAMS": "1"}


def comb_tree(V, P, d, g=0.6, seed=0x5EED0300):
    """x = voice + g * Delay(x, d), one loop per voice (the patch of tools/feedback_bench.py)."""
    gr = synth.GraphArrays()
    p = synth.voice_params(V, P, seed, wrap=64)
    voices = synth.sum_tree(gr, synth.partial_leaves(gr, p["w"], p["amp"]).reshape(V, P))
    x = gr.nodes(synth.K_SUM2, V)
    dl = gr.nodes(synth.K_DELAY, V)
    m = gr.binop(synth.K_MUL, dl, synth.C(np.float32(g)), V)
    gr.edge(voices, x, 0, 0)
    gr.edge(m, x, 0, 1)
    gr.edge(x, dl, 0, 0)
    gr.const(dl, np.float32(d), 1)
    gr.edge(x, 0, 0, np.arange(V, dtype=np.uint32))
    return gr.finish(V)


def mix_tree(V, P, base_delay=2400.0):
    """Row v = tap(voice v) + tap(voice (v + 1) % V): every row needs two voices of the same block (a mix bus)."""
    p = synth.voice_params(V, P, 0x5EED0003, True)
    g = synth.GraphArrays()
    x = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))
    x = synth.delay_chain(g, x, 1, base_delay)
    y = g.binop(synth.K_SUM2, x, np.roll(x, -1), V)
    g.edge(y, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


# (name, builder, voices, programs per voice, shortest delayed read of a ring that a PROGRAM stores).  The last one from the
# graph: behind an envelope every tap reads a program's value (env * voice, then the taps before it), so the shortest is the
# first tap's base_delay; without the envelope the first tap reads the bare voice's ring, which the bank stores, and the
# shortest is the second tap's 2 * base_delay; no taps: none (0); a comb reads its own loop d frames back.
SERVABLE = [
    ("effects_2x128", lambda: synth.effects_tree(2, 128), 2, 1, 2400),
    ("effects_4x256", lambda: synth.effects_tree(4, 256), 4, 1, 2400),
    ("effects_3x1024_two_taps", lambda: synth.effects_tree(3, 1024, taps=2, base_delay=100.0), 3, 1, 100),
    ("effects_64x1024", lambda: synth.effects_tree(64, 1024), 64, 1, 2400),
    ("envelope_only", lambda: synth.effects_tree(4, 256, taps=0), 4, 1, 0),
    ("taps_only", lambda: synth.effects_tree(4, 256, envelope=False), 4, 1, 4800),
    ("taps_only_64", lambda: synth.effects_tree(2, 128, envelope=False, taps=3, base_delay=64.0), 2, 1, 128),
    ("comb_64", lambda: comb_tree(4, 256, 64), 4, 1, 64),
    ("comb_441", lambda: comb_tree(16, 1024, 441), 16, 1, 441),
    ("comb_2400", lambda: comb_tree(2, 128, 2400), 2, 1, 2400),
]

# (name, builder, voices, fragment of the reason)
REFUSED = [
    ("comb_63", lambda: comb_tree(4, 256, 63), 4, "63 frames back"),
    ("comb_32", lambda: comb_tree(4, 256, 32), 4, "32 frames back"),
    ("base_delay_32", lambda: synth.effects_tree(4, 256, base_delay=32.0), 4, "less than 64 frames back"),
    ("mix_row", lambda: mix_tree(2, 256), 2, "mix bus"),
    ("chorus", lambda: synth.chorus_tree(2, 256), 2, "S_READ_DYN"),
    ("small_voices", lambda: synth.effects_tree(2, 64), 2, "at least 128 partials"),
    ("more_voices_than_cus", lambda: synth.effects_tree(300, 128, taps=1), 300, "one voice per CU"),
]


def case(table, name):
    for c in table:
        if c[0] == name:
            return c
    raise KeyError(name)


# ---- block sequences on the device (tests/test_hip_stream_programs.py) ---------------------------------------------------

SPECIAL = np.array([0.0, -0.0, -1.0, 0.5, 1e-42, 16777216.0, 4294967296.0, 4294967808.0, 1e30, np.inf, -np.inf, np.nan], np.float32)
# (the resident launch ends itself after this long without a block; nothing else runs between two blocks of a sequence)
STREAM_OPTIONS = dict(OPTION, FR_STREAM_IDLE_MS="1500")


def block_rows(rng, starts):
    """[(idx, row)] for blocks of random length 1..64 from each start in `starts` = [(first frame, frames to cover)]; every
    fifth block carries hostile time values."""
    rows, k = [], 0
    for idx, frames in starts:
        end = idx + frames
        while idx < end:
            T = int(min(rng.integers(1, 65), end - idx))
            row = synth.time_ramp(idx, idx + T)
            if k % 5 == 4:
                row = row.copy()
                row[rng.integers(T, size=max(1, T // 4))] = SPECIAL[rng.integers(len(SPECIAL), size=max(1, T // 4))]
            rows.append((idx, row))
            idx += T
            k += 1
    return rows


FIRST_LENGTHS = (64, 64, 1, 37, 64, 2, 63)      # full, full, one frame, ragged, full, two, one short of full
FINITE_SPECIAL = SPECIAL[np.isfinite(SPECIAL)]  # every one of them gives a finite voice
POISON = SPECIAL[~np.isfinite(SPECIAL)]


def finite_block_rows(rng, starts):
    """[(idx, row)] as block_rows gives them, for patches with feedback: in x = voice + g * Delay(x, d) a NaN never leaves, so
    rows that poison a loop early leave NaN to be compared with NaN.  Per segment of `starts` = [(first frame, frames)]: the
    first seven blocks have FIRST_LENGTHS, the later ones a random length 1..64, the last one is cut at the segment's end;
    every fifth block (k % 5 == 4) carries hostile but FINITE time values in a quarter of its entries; the segment's last
    block carries +-inf and NaN in a quarter of its entries -- what follows it is a seek (the engine rebuilds the loops from
    frame 0 with every input 0.0) or the end."""
    rows = []
    for idx, frames in starts:
        end, k = idx + frames, 0
        while idx < end:
            T = int(min(FIRST_LENGTHS[k] if k < len(FIRST_LENGTHS) else rng.integers(1, 65), end - idx))
            row = synth.time_ramp(idx, idx + T)
            values = POISON if idx + T == end else FINITE_SPECIAL if k % 5 == 4 else None
            if values is not None:
                row = row.copy()
                row[rng.integers(T, size=max(1, T // 4))] = values[rng.integers(len(values), size=max(1, T // 4))]
            rows.append((idx, row))
            idx += T
            k += 1
    return rows


def silence_voice(tree, V, P, v):
    """The tree with every amplitude of voice v of its bank of V voices x P partials (synth.voice_params: amp = 1 / (k + 1))
    replaced by +0.0: every leaf of the voice is +-0, every chunk sum of it is an exact zero, and the kernel has to find the
    zero's sign from the leaves.  The amplitudes are the one batch of V * P constant edges into slot 0 of consecutive nodes
    that holds exactly these values."""
    want = synth.bits(np.tile(synth.voice_params(V, P, 0)["amp"][0], V))
    e = tree["edges"].copy()
    n = V * P
    const = (e[:, 0] == synth.CONST_HANDLE) & (e[:, 3] == 0)
    follows = np.concatenate([[False], const[1:] & const[:-1] & (e[1:, 1] == e[:-1, 1] + 1)])   # edge i continues edge i - 1's batch
    for i in np.nonzero(const & ~follows)[0]:                                                   # where a batch begins
        if i + n <= len(e) and follows[i + 1:i + n].all() and not (i + n < len(e) and follows[i + n]) and np.array_equal(e[i:i + n, 2], want):
            e[i + v * P:i + (v + 1) * P, 2] = 0
            return dict(tree, edges=e)
    raise ValueError(f"no bank of {V} x {P} amplitudes in this tree")


def short_blocks(idx=200, lengths=(64, 1, 37)):
    """[(idx, row)]: a full block, a block of one frame and a last block shorter than 64 frames, one after the other."""
    rows = []
    for T in lengths:
        rows.append((idx, synth.time_ramp(idx, idx + T)))
        idx += T
    return rows


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def first_diff(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    bad = np.argwhere(~((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    if len(bad) == 0:
        return "identical"
    i = tuple(bad[0])
    return f"{len(bad)} of {a.size} differ; first at {i}: got {a[i]!r} expected {b[i]!r}"


def stream_against_fill_buffer(hip_lib, tree, V, rows, semantics="reference"):
    """The blocks through fr_stream_block of a renderer with the option on, then the same blocks through fr_fill_buffer of a
    second renderer with the option off; every sample of every block equal bit for bit.  The second renderer renders after
    the stream is closed: while a resident launch runs, other work of the process may be queued behind it (streams share
    the device's few hardware queues) and would wait until the launch ends itself.
    Returns [(idx, streamed block)] and the streaming renderer's plan."""
    from libfriendship_amd.capi import Renderer
    with Renderer(hip_lib, semantics=semantics, options=STREAM_OPTIONS) as s:
        synth.install(s, tree)
        s.stream_begin(V)
        got = [(idx, s.stream_block(idx, row)) for idx, row in rows]
        plan = s.plan()
        s.stream_end()
    with Renderer(hip_lib, semantics=semantics) as f:
        synth.install(f, tree)
        for k, ((idx, row), (_, a)) in enumerate(zip(rows, got)):
            b = f.fill_buffer(V, idx, idx + len(row), [row])
            assert same_bits(a, b), f"block {k} at frame {idx} (T={len(row)}): " + first_diff(a, b)
    return got, plan
