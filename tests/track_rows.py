"""The input matrices of the track-voice cases (tests/track_variants.py) and what the dense reference expects of them:
shared by tests/test_track_variants.py (CPU: the conditions the matrices must meet, the span sequences against the oracle)
and tests/test_hip_track_matrix.py (GPU).  Plain numpy, no GPU.

A call of synth.track_tree(V, P) takes a dense matrix [1 + 2 V P, T]: row 0 the time row, then per partial its w row and its
amp row.  Regular rows are random per element (a kernel that reads another frame, another partial or another piece's rows
gets other values), small positive w and amplitudes 1/(k+1) scaled by 0.5 .. 1.5."""
import numpy as np

import bank_reference
from libfriendship_amd import synth
from libfriendship_amd.synth import K_DELAY, C

_F = np.float32
OFFSET = (1 << 20) + 37

# negative, -0, NaN, +-inf, huge, subnormals; t * w integral (1, 0.5 at even frames, -2) or beyond 2^23 at OFFSET (16, 8)
HOSTILE_W = np.array([-0.013, -0.0, np.nan, np.inf, -np.inf, 1e30, 1e-45, -3e-39, 1.0, 0.5, 16.0, -2.0, 3e38, 0.25, -1e-30, 8.0, 0.0], _F)
HOSTILE_AMP = np.array([0.0, -0.0, -0.7, np.nan, np.inf, -np.inf, 1e-45, -3e-39, 3e38, -1.0, 0.0, -0.0, 2.5], _F)
# the time row's hostile values, as tests/test_hip_bank_matrix.py hostile_row places them
HOSTILE_NEG = np.array([-1e-9, -1e-30, -1e-45, -1e-20, -0.3, -2.5, -1e-7, -0.75, -3e-39, -1.5e-8, -0.001, -17.25], _F)
HOSTILE_ODD = np.array([np.nan, np.inf, -np.inf, 1e30, 3e38, 4294967296.0, 8e9, -0.0, 1e-45, 3e-39, 0.625, 2.5e-7], _F)


def regular_rows(V, P, idx, T, seed):
    """The matrix of a call at frame idx: the time ramp and regular track rows."""
    rng = np.random.default_rng([seed, idx, T])
    n = V * P
    m = np.empty((1 + 2 * n, T), _F)
    m[0] = synth.time_ramp(idx, idx + T)
    m[1::2] = rng.random((n, T), dtype=_F) * _F(0.05)
    m[2::2] = (rng.random((n, T), dtype=_F) + _F(0.5)) * np.tile(_F(1.0) / np.arange(1, P + 1, dtype=_F), V)[:, None]
    return m


def hostile_time(idx, T):
    """The ramp with a wave of negative times (frames 69 ..) and a later wave of the other hostile values (.. T - 2)."""
    row = synth.time_ramp(idx, idx + T)
    a = min(69, T - len(HOSTILE_NEG))
    row[a:a + len(HOSTILE_NEG)] = HOSTILE_NEG
    b = T - len(HOSTILE_ODD) - 1
    if b >= a + len(HOSTILE_NEG):
        row[b:b + len(HOSTILE_ODD)] = HOSTILE_ODD
    return row


def hostile_spots(case):
    """[(voice, first leaf, leaves)] of the hostile call: in voice 0 the first 8-leaf group, the last one (the prefetched one
    wherever a wave has two), and the last group of a piece -- of a wave's share where voices are whole -- that is not the
    voice's last; in voice V - 1 the whole share of one wave and of no other (wave 1 of piece 0; whole voices per wave: the
    voice)."""
    V, P = case["V"], case["P"]
    piece = P >> case["pieces_log2"]
    share = P if case["key"] == "jit_bank_multi" else piece // 4
    inner = piece if case["pieces_log2"] else share
    spots = [(0, 0, 8), (0, P - 8, 8)]
    if inner < P:
        spots.append((0, inner - 8, 8))
    spots.append((V - 1, 0 if share == P else share, share))
    return spots


def hostile_frames(T):
    """Frame T - 1 is the one the lanes past the call's end re-read; 63 and 64 the edge of the first tile."""
    return sorted({0, 63, 64, T // 2, T - 1} & set(range(T)))


def hostile_rows(case, idx, seed):
    """(matrix, hostile voices) of the hostile call: regular rows, the hostile time row, and hostile w / amp values at
    hostile_spots x hostile_frames -- two voices and five frames at the most."""
    V, P, T = case["V"], case["P"], case["T"]
    m = regular_rows(V, P, idx, T, seed)
    m[0] = hostile_time(idx, T)
    frames = hostile_frames(T)
    for v, k0, n in hostile_spots(case):
        for k in range(k0, k0 + n):
            slot = 1 + 2 * (v * P + k)
            for j, f in enumerate(frames):
                m[slot, f] = HOSTILE_W[(k + 3 * j) % len(HOSTILE_W)]
                m[slot + 1, f] = HOSTILE_AMP[(5 * k + j) % len(HOSTILE_AMP)]
    return m, sorted({0, V - 1})


class SlotLimit:
    """The reference's input vectors: n_slots * n_times of the largest call so far; rows at or beyond are dropped."""

    def __init__(self):
        self.n_vecs = 0

    def call(self, n_slots, n_times):
        self.n_vecs = max(self.n_vecs, n_slots * n_times)
        return self.n_vecs


def expected(V, P, m, limit=None):
    """The dense reference's output [V, T] of a call with matrix m under the slot limit."""
    w, amp = bank_reference.track_params(m, V, P, limit)
    return bank_reference.render_track_bank(w, amp, m[0])


def quiet_voices_sound(exp, hostile=()):
    """'' when every voice outside `hostile` is finite and nonzero in at least half its samples, else which one is not."""
    for v in range(exp.shape[0]):
        if v in hostile:
            continue
        good = int((np.isfinite(exp[v]) & (exp[v] != 0)).sum())
        if 2 * good < exp.shape[1]:
            return f"voice {v}: {good} of {exp.shape[1]} samples finite and nonzero"
    return ""


def priming_slots(V, P, T):
    """Output slots to request so that a T-frame call makes every row live: n_slots * T >= 1 + 2 V P."""
    return max(V, -(-(1 + 2 * V * P) // T))


# ---- ring spans ---------------------------------------------------------------------------------------------------------
def span_tree(V, P, d):
    """out_v = Delay(voice_v, d) over synth.track_tree's voices."""
    g = synth.GraphArrays()
    w_slots = 1 + 2 * np.arange(V * P, dtype=np.uint32)
    roots = synth.sum_tree(g, synth.track_leaves(g, w_slots, w_slots + 1).reshape(V, P))
    out = g.binop(K_DELAY, roots, C(np.full(V, d, _F)), V)
    g.edge(out, 0, 0, np.arange(V, dtype=np.uint32))
    t = g.finish(V)
    t["n_inputs"] = 1 + 2 * V * P
    return t


def span_rows(V, P, idx, T, seed):
    """Regular rows; the time row holds small frame numbers here, so scale w up to keep the voices sounding."""
    m = regular_rows(V, P, idx, T, seed)
    m[1::2] *= _F(3.0)
    return m


class SpanReference:
    """The dense reference over absolute frames: voice_v[t] from frame t's rows (rows the slot limit dropped and every frame
    before a seek read +0, which makes the voice +0 as well: 0 * parab(0)), and out_v[t] = voice_v[t - d], 0 before frame 0."""

    def __init__(self, V, P, d):
        self.V, self.P, self.d = V, P, d
        self.limit = SlotLimit()
        self.head = 0
        self.past = np.zeros((V, d), _F)      # voice_v over [head - d, head)

    def call(self, idx, m, n_slots=None):
        V, d = self.V, self.d
        T = m.shape[1]
        if idx != self.head:
            self.past = np.zeros((V, d), _F)
        voice = expected(V, self.P, m, self.limit.call(V if n_slots is None else n_slots, T))
        both = np.concatenate([self.past, voice], axis=1)
        self.past = both[:, T:]
        self.head = idx + T
        return both[:, :T]


def span_launches(idx, n, d, head, cap):
    """The frames of each bank launch of a call, from the rules of callplan.hpp (delay rings of max(1024, pow2 >= d + n)
    frames; a call that grows them, or that does not continue the last one, renders [idx - d, idx + n)) and engine.cpp
    launch_bank_window (the part before idx in spans cut where the 64-frame history ring wraps, then the call's frames).
    `head`, `cap`: the end of the call before and the rings' capacity.  Returns (frames per launch, the capacity after)."""
    need = 1024
    while need < d + n:
        need <<= 1
    valid = idx == head and need <= cap
    s = idx if valid else max(0, idx - d)
    frames = []
    while s < idx:
        frames.append(min(idx - s, 64 - (s & 63)))
        s += frames[-1]
    return frames + [n], max(cap, need)
