"""A partial-block-sharded job (shard_harness.Job, FR_SHARD_PARTIALS) driven through a call sequence that takes every
branch of the time-tiled exchange at its DEFAULT geometry (csrc/callplan.hpp exchange_tiles: at most 4 tiles, none shorter than
1024 frames, 64-aligned), checked against the oracle by sampling.  Shared by the CPU twin on the host-logic simulator
(test_shard_sim.py) and the HIP tests (test_hip_shard.py): the same calls, the same frame choice, the same assertions.

The sequence: two contiguous 4800-frame calls (the second is steady for ring plans: its row is deferred to the bank
kernels and appended tile by tile), a ragged call, a call of two tiles, one below the minimum tile, a 2-frame call, a
graph edit (a ring plan then rebuilds its look-back window from the history the tiles appended), a backward seek (a ring
plan's window starts lmax frames early, so the call's first frame falls inside a tile: the final combine's `out_skip`),
and a device-resident call.  Some rows are the ramp + 0.5, so that history appended at a wrong offset cannot match."""
import numpy as np

from kat_replay import same_bits
from libfriendship_amd import synth
from test_hip_parity import _sampled_parity, first_diff

MAX_TILES, MIN_TILE = 4, 1024     # engine.cpp x_max_tiles / x_min_tile defaults
SENTINEL = np.float32(-12345.0)


def exchange_tiles(xlen, max_tiles=MAX_TILES, min_tile=MIN_TILE):
    """(offset in the window, frames) of every tile, as callplan.hpp exchange_tiles cuts an exchange window of xlen frames."""
    nt = max(1, min(max_tiles, xlen // max(min_tile, 64)))
    tl = ((xlen + nt - 1) // nt + 63) // 64 * 64
    return [(off, min(tl, xlen - off)) for off in range(0, xlen, tl)]


class Window:
    """The window callplan.hpp call_windows has the split voices rendered over: the call's frames, or -- when split voices feed rings that do
    not hold [idx - lmax, idx) of the current graph (first call, seek, edit, ring growth) -- [idx - lmax, idx + n)."""

    def __init__(self, lmax=None):
        self.lmax, self.cap, self.end = lmax, 0, None

    def __call__(self, idx, n):
        if self.lmax is None:
            return idx, n
        cap = 1024
        while cap < self.lmax + n:
            cap <<= 1
        steady = self.end == idx and cap <= self.cap
        self.cap, self.end = max(self.cap, cap), idx + n
        if steady:
            return idx, n
        w0 = idx - self.lmax if idx > self.lmax else 0
        return w0, idx + n - w0

    def invalidate(self):
        self.end = None


class Call:
    def __init__(self, start, n, offset=0.0, device=False, edit=False):
        self.start, self.n, self.offset, self.device, self.edit = start, n, offset, device, edit

    def row(self):
        return (synth.time_ramp(self.start, self.start + self.n) + np.float32(self.offset)).astype(np.float32)

    def __repr__(self):
        return f"[{self.start}, {self.start + self.n}){' +%g' % self.offset if self.offset else ''}{' device' if self.device else ''}" \
               f"{' after an edit' if self.edit else ''}"


def standard_calls(lmax=0, first=4800):
    """The sequence above.  `lmax`: the tree's look-back (the seek goes to a frame with a full look-back window)."""
    calls, t = [], 0

    def add(n, **kw):
        nonlocal t
        calls.append(Call(t, n, **kw))
        t += n
    add(first)
    add(4800, offset=0.5)
    add(4777)
    add(2100, offset=0.5)
    add(1023)
    add(2)
    add(4800, edit=True)
    add(4800, offset=0.5)
    seek = max(16000, lmax + 1000)
    assert seek + 3000 < t
    t = seek
    add(3000, offset=0.5)
    add(4800, device=True)
    return calls


def sample_frames(call, x0, xlen, rng, lags=()):
    """Frames of the call to compare: 0, 1, 63, 64, T-1, both sides of every tile boundary, frames that read a tile
    boundary through a delay `lag`, a few random ones."""
    a, b = call.start, call.start + call.n
    fr = [a + k for k in (0, 1, 63, 64, call.n - 1)]
    for off, _ in exchange_tiles(xlen)[1:]:
        for d in (0,) + tuple(lags):
            fr += [x0 + off + d - 1, x0 + off + d, x0 + off + d + 1]
    fr += list(rng.integers(a, b, 3))
    return np.unique([f for f in fr if a <= f < b]).astype(np.uint64)


class SampledOracle:
    """The oracle holding the tree, checked call by call: the call's row is stored with the output edges removed (no
    render), the edges go back, and the call's sampled (slot, frame) pairs are evaluated against that history."""

    def __init__(self, ref, tree):
        self.ref = ref
        e = tree["edges"]
        self.out = [tuple(int(x) for x in r) for r in e[e[:, 1] == 0]]
        synth.install(ref, dict(tree, edges=e[e[:, 1] != 0]))

    def edit(self, dele, add):
        self.out.remove(tuple(dele))
        self.out.append(tuple(add))

    def check(self, call, got, slots, frames, what):
        assert not self.ref.fill_buffer(1, call.start, call.start + call.n, [call.row()]).any()
        self.ref.on_add_edges(np.array(self.out, dtype=np.uint32))
        try:
            _sampled_parity(self.ref, [(call.start, got)], slots, frames, what)
        finally:
            for e in self.out:
                self.ref.on_del_edge(*e)


def output_edit(tree, n_slots):
    """The edit of the sequence: the last row is rewired to whatever feeds the row before it."""
    e = tree["edges"]
    last = [int(x) for x in e[(e[:, 1] == 0) & (e[:, 3] == n_slots - 1)][0]]
    prev = [int(x) for x in e[(e[:, 1] == 0) & (e[:, 3] == n_slots - 2)][0]]
    return last, [prev[0], 0, prev[2], n_slots - 1]


def half_delayed_tree(n_voices, n_partials, taps=3, base_delay=400.0, seed=0x5EED0005):
    """Even voices through a delay chain (their mixes go to rings), odd voices straight to their rows.  Split voices of
    both kinds share one exchange window: after a seek it starts lmax frames before the call, and the finished direct
    voices skip the look-back part of the tile the call starts in (the final combine's out_skip)."""
    p = synth.voice_params(n_voices, n_partials, seed, detune=True)
    g = synth.GraphArrays()
    roots = synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(n_voices, n_partials))
    for v in range(n_voices):
        x = synth.delay_chain(g, roots[v:v + 1], taps, base_delay) if v % 2 == 0 else roots[v:v + 1]
        g.edge(x, 0, 0, v)
    return g.finish(n_voices)


def host_device_fill(ren, n_slots, call):
    """fr_fill_buffer_device on the simulator, whose 'device' memory is host memory."""
    out = np.full((n_slots, call.n), SENTINEL, dtype=np.float32)
    row = call.row()
    ren.fill_buffer_device(out.ctypes.data, n_slots, call.n, call.start, row.ctypes.data, [0, call.n], 0)
    return out


def run(job, ref, tree, n_slots, calls, slots=None, lmax=None, lags=(), serial=None, device_fill=host_device_fill, seed=0):
    """Every call on every rank of `job` (and of `serial`, a FR_SHARD_SERIAL_EXCHANGE job given the same calls, if any):
    the assembled rows against the oracle at sample_frames(), nobody writing rows it does not own, each call's exchange
    cut into the tiles exchange_tiles() predicts, the tiled and the serial job bit-identical and sending the same bytes.
    Returns every rank's plan after the first call (before the edit) and after the last."""
    rng = np.random.default_rng(seed)
    slots = np.arange(n_slots) if slots is None else np.asarray(slots)
    oracle = SampledOracle(ref, tree)
    window = Window(lmax)
    edit = output_edit(tree, n_slots)
    stats = lambda j: [r.plan().get("exchange_stats", {"calls": 0, "tiles": 0, "bytes_sent": 0}) for r in j.ranks]
    before = stats(job)
    for k, call in enumerate(calls):
        what = f"call {k} {call}"
        if call.edit:
            for ren in job.ranks + (serial.ranks if serial else []):
                ren.on_del_edge(*edit[0])
                ren.on_add_edge(*edit[1])
            oracle.edit(*edit)
            window.invalidate()
        if call.device:
            bufs = job.each(lambda _r, ren: device_fill(ren, n_slots, call))
        else:
            bufs = job.fill(n_slots, call.start, call.start + call.n, [call.row()], sentinel=SENTINEL)
        got = job.assemble(bufs, n_slots, sentinel=SENTINEL)
        x0, xlen = window(call.start, call.n)
        tiles = exchange_tiles(xlen)
        for r, (s0, s1) in enumerate(zip(before, stats(job))):
            assert (s1["calls"] - s0["calls"], s1["tiles"] - s0["tiles"]) == (1, len(tiles)), \
                f"{what}, rank {r}: window [{x0}, {x0 + xlen}) should be {len(tiles)} tiles {tiles}: {s0} -> {s1}"
        before = stats(job)
        if k == 0:
            first_plans = [r.plan() for r in job.ranks]
        if serial is not None:
            sbufs = (serial.each(lambda _r, ren: device_fill(ren, n_slots, call)) if call.device else
                     serial.fill(n_slots, call.start, call.start + call.n, [call.row()], sentinel=SENTINEL))
            sgot = serial.assemble(sbufs, n_slots, sentinel=SENTINEL)
            assert same_bits(got, sgot), f"{what}: tiled vs serial exchange: " + first_diff(got, sgot)
        frames = sample_frames(call, x0, xlen, rng, lags)
        oracle.check(call, got, slots, frames, what)
    if serial is not None:
        st, ss = stats(job), stats(serial)
        assert [s["bytes_sent"] for s in st] == [s["bytes_sent"] for s in ss], (st, ss)
        assert all(s["tiles"] == s["calls"] == len(calls) for s in ss), ss
        assert sum(job.boxes.bytes_sent) == sum(serial.boxes.bytes_sent)
    return first_plans, [r.plan() for r in job.ranks]
