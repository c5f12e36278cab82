"""Dense f32 reference of partial-form oscillator banks, for tests.

out[v, t] = TREE_k amp[v, k] * parab(Modulo(t * w[v, k], 1)), with the 11-node partial of synth.partial_leaves and the
sum_tree association (adjacent pairs level by level, an odd element carried up unchanged): the f32 operations of
synth.bank_reference_numpy in the same order, over many voices at once.  Voices and frames are processed in slices so that no
temporary grows beyond about `budget` elements.  tests/test_bank_variants.py pins it bit for bit to the C++ oracle.

Only the sum_tree association is restated here.  For any other Sum2 tree over the same leaves -- chains, unbalanced trees, DAGs:
what the schedule kernels render item by item -- the dense reference is tests/tree_shapes.py render_shapes, which takes its
leaves from _leaves and adds them in each tree's own association (pinned to the oracle by tests/test_tree_shapes.py).

render_track_bank is the same bank with w and amp given per frame (control-rate tracks, synth.track_leaves: w[v, k, t] and
amp[v, k, t] read from input rows); track_params cuts them out of a call's dense input matrix under the slot limit of the
call.  tests/test_track_variants.py pins both to the oracle."""
import numpy as np

_F = np.float32


def _leaves(w, amp, t):
    """w, amp: [v, P] (constants) or [v, P, T] (per frame); t: [T] -> leaves [v, P, T]."""
    if w.ndim == 2:
        w, amp = w[:, :, None], amp[:, :, None]
    with np.errstate(all="ignore"):
        x = t[None, None, :] * w
        # fmod(x, 1) as x - trunc(x): exact for every finite x and NaN for +-inf and NaN, like fmodf; it differs only in the
        # sign of a zero remainder (fmodf(-3, 1) = -0), which u = ph + (-0.5) discards.  (np.fmod costs 30x as much.)
        rem = x - np.trunc(x)
        ph = np.where(rem < 0, rem + _F(1.0), rem)
        u = ph + _F(-0.5)
        nu = _F(-1.0) * u
        m = np.where((u < nu) | np.isnan(nu), u, nu)
        ab = _F(-1.0) * m
        n1 = _F(-1.0) * ab
        q = _F(0.5) + n1
        pp = _F(-16.0) * u
        y = pp * q
        return amp * y


def _tree(cur):
    """Sum over axis 1 in the sum_tree association."""
    while cur.shape[1] > 1:
        npair = cur.shape[1] // 2
        with np.errstate(all="ignore"):
            s = cur[:, 0:2 * npair:2] + cur[:, 1:2 * npair:2]
        cur = np.concatenate([s, cur[:, 2 * npair:]], axis=1) if cur.shape[1] % 2 else s
    return cur[:, 0]


def render_bank(w, amp, t, budget=1 << 22):
    """w, amp: [V, P] f32; t: [T] f32 -> [V, T] f32."""
    w = np.ascontiguousarray(w, _F)
    amp = np.ascontiguousarray(amp, _F)
    t = np.ascontiguousarray(t, _F)
    V, P = w.shape
    T = len(t)
    out = np.empty((V, T), _F)
    if V == 0 or T == 0:
        return out
    tstep = max(1, min(T, budget // P))
    vstep = max(1, budget // (P * tstep))
    for v0 in range(0, V, vstep):
        for t0 in range(0, T, tstep):
            out[v0:v0 + vstep, t0:t0 + tstep] = _tree(_leaves(w[v0:v0 + vstep], amp[v0:v0 + vstep], t[t0:t0 + tstep]))
    return out


def render_track_bank(w, amp, t, budget=1 << 22):
    """w, amp: [V, P, T] f32, the values of frame t's rows; t: [T] f32 -> [V, T] f32.  The 11-node partial of
    synth.track_leaves (the operations of _leaves, amp the FIRST operand of the last product as there) under sum_tree."""
    w = np.asarray(w, _F)
    amp = np.asarray(amp, _F)
    t = np.ascontiguousarray(t, _F)
    V, P, T = w.shape
    assert amp.shape == w.shape and t.shape == (T,), (w.shape, amp.shape, t.shape)
    out = np.empty((V, T), _F)
    if V == 0 or T == 0:
        return out
    tstep = max(1, min(T, budget // P))
    vstep = max(1, budget // (P * tstep))
    for v0 in range(0, V, vstep):
        for t0 in range(0, T, tstep):
            out[v0:v0 + vstep, t0:t0 + tstep] = _tree(_leaves(w[v0:v0 + vstep, :, t0:t0 + tstep], amp[v0:v0 + vstep, :, t0:t0 + tstep],
                                                              t[t0:t0 + tstep]))
    return out


def track_params(m, V, P, limit=None, first_track=1):
    """(w, amp), each [V, P, T], of a call of synth.track_tree(V, P, first_track=first_track) whose dense input matrix is
    m [rows, T]: partial k of voice v reads w from slot first_track + 2 (v P + k) and amp from the next one.  Slots at or
    beyond `limit` (the rows the call's slot limit drops; default: the matrix's rows) read +0.0."""
    m = np.asarray(m, _F)
    T = m.shape[1]
    limit = m.shape[0] if limit is None else min(int(limit), m.shape[0])
    rows = np.zeros((2 * V * P, T), _F)
    have = max(0, min(limit - first_track, 2 * V * P))
    rows[:have] = m[first_track:first_track + have]
    rows = rows.reshape(V, P, 2, T)
    return rows[:, :, 0, :], rows[:, :, 1, :]


def bank_tree(w, amp, time_slot=0):
    """The graph of the same bank, one output slot per voice (synth.partial_leaves + synth.sum_tree)."""
    from libfriendship_amd import synth
    w = np.asarray(w, _F)
    V, P = w.shape
    g = synth.GraphArrays()
    leaves = synth.partial_leaves(g, w, np.asarray(amp, _F), time_slot).reshape(V, P)
    g.edge(synth.sum_tree(g, leaves), 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def first_diff(got, exp, what=""):
    """'' when every sample has the same bits (NaN == NaN); else where and how the first one differs."""
    got = np.asarray(got, _F)
    exp = np.asarray(exp, _F)
    if got.shape != exp.shape:
        return f"{what}: shape {got.shape} != {exp.shape}"
    bad = ~((got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp)))
    if not bad.any():
        return ""
    v, f = (int(i) for i in np.argwhere(bad)[0])
    return (f"{what}: {int(bad.sum())} of {bad.size} samples differ; first at voice {v}, frame {f}: got {got[v, f]!r} "
            f"({got.view(np.uint32)[v, f]:#010x}) expected {exp[v, f]!r} ({exp.view(np.uint32)[v, f]:#010x})")
