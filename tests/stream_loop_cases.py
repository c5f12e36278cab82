"""Patches for block streaming of feedback loops shorter than a block (FR_STREAM_LOOPS on top of FR_STREAM_PROGRAMS), shared by
the simulator tests of the serving rule (tests/test_stream_loops_sim.py) and the GPU tests of the resident kernel
(tests/test_hip_stream_loops.py).  Graph recipes and plain data: importable without a GPU.

Expectations come from the graph:
  * a comb x = voice + g * Delay(x, d) is one loop program per voice with stride d (d < 64; d >= 64 is no loop program: an
    earlier block stored what it reads);
  * a loop with several taps x = voice + g1 * Delay(x, d1) + g2 * Delay(x, d2) strides by the gcd of the taps below 64 frames:
    (2, 3) -> 1, (6, 9) -> 3, (3, 441) -> 3;
  * what reads a loop's ring behind it (a tap Delay(x, 2), a second row that is x itself) is a further program of the SAME
    voice with stride 0;
  * a loop behind a sum of several voices is a bus program (FR_STREAM_BUS); a sum of several voices' loops inlines the loops
    and is one bus program whose stride is the gcd of all of them.

The oracle evaluates a loop by recursion without a memo, so a frame t of a loop with taps d1, d2, ... costs
c(t) = 1 + c(t - d1) + c(t - d2) + ... voice evaluations (a comb: t / d + 1).  `oracle_frames(delays)` is the number of leading
frames whose summed cost stays within ORACLE_BUDGET = 20 000 voice evaluations per voice: comb(1) 199, comb(5) 444, comb(32)
1115, comb(63) 1556, taps (2, 3) 29, (6, 9) 76, (3, 441) 344, the tap behind comb(5) with its two rows 313.  Up to there the
streamed blocks are also compared with the oracle; the comparison with fr_fill_buffer covers every sample."""
import numpy as np

import stream_bus_cases as B
import stream_cases as K
import stream_input_cases as I
from libfriendship_amd import synth
from stream_cases import block_rows, comb_tree, finite_block_rows, short_blocks, silence_voice   # noqa: F401  (the tests take them from here)

NEW_KERNEL = "bank_stream_loops_kernel"
PROGRAMS = dict(K.OPTION)                                       # FR_STREAM_PROGRAMS alone
OPTION = dict(PROGRAMS, FR_STREAM_LOOPS="1")
BUS = dict(OPTION, FR_STREAM_BUS="1")
INPUTS = dict(OPTION, FR_STREAM_INPUTS="1")
BANKS = dict(OPTION, FR_STREAM_BANKS="1")
IDLE = {"FR_STREAM_IDLE_MS": "1500"}                            # (as stream_cases.STREAM_OPTIONS)
LOOP_LOADS, LOOP_STORES = 32, 16                                # csrc/streamplan.hpp STREAM_LOOP_LOADS / STREAM_LOOP_STORES
ORACLE_BUDGET = 20000


def oracle_frames(delays, budget=ORACLE_BUDGET):
    cost, total, t = [], 0, 0
    while True:
        c = 1 + sum(cost[t - d] for d in delays if t >= d)
        if total + c > budget:
            return t
        cost.append(c)
        total += c
        t += 1


def _voices(g, V, P, seed=0x5EED0800):
    p = synth.voice_params(V, P, seed, wrap=64)
    return synth.sum_tree(g, synth.partial_leaves(g, p["w"], p["amp"]).reshape(V, P))


def _loop(g, src, taps, n):
    """x = src + sum over (d, gain) of gain * Delay(x, d), one loop per element of src (Sum2 chain: src, then the taps in order)."""
    dls, x = [], None
    acc = src
    for k, (d, gain) in enumerate(taps):
        dl = g.nodes(synth.K_DELAY, n)
        g.const(dl, np.float32(d), 1)
        m = g.binop(synth.K_MUL, dl, synth.C(np.float32(gain)), n)
        x = g.nodes(synth.K_SUM2, n)
        g.edge(acc, x, 0, 0)
        g.edge(m, x, 0, 1)
        acc = x
        dls.append(dl)
    for dl in dls:
        g.edge(x, dl, 0, 0)
    return x


def taps_tree(V, P, delays, gains=(0.45, -0.35)):
    """x = voice + 0.45 * Delay(x, d1) - 0.35 * Delay(x, d2): own reads at several delays, one loop per voice."""
    g = synth.GraphArrays()
    x = _loop(g, _voices(g, V, P), list(zip(delays, gains)), V)
    g.edge(x, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def tap_behind_tree(V, P):
    """x = voice + 0.75 * Delay(x, 5); row v = Delay(x, 2), row V + v = x itself (a row copy)."""
    g = synth.GraphArrays()
    x = _loop(g, _voices(g, V, P), [(5, 0.75)], V)
    tap = g.binop(synth.K_DELAY, x, synth.C(np.float32(2.0)), V)
    g.edge(tap, 0, 0, np.arange(V, dtype=np.uint32))
    g.edge(x, 0, 0, V + np.arange(V, dtype=np.uint32))
    return g.finish(2 * V)


def arith_tree(V, P):
    """loop_tile_cases.arith_loop behind a voice: x = voice + Minimum(Modulo(Divide(Multiply(Delay(x, 1), 0.5), In(1)), 1.5),
    voice), the control row In(1) as the divisor."""
    g = synth.GraphArrays()
    v = _voices(g, V, P)
    x = g.nodes(synth.K_SUM2, V)
    dl = g.nodes(synth.K_DELAY, V)
    g.const(dl, np.float32(1.0), 1)
    g.edge(x, dl, 0, 0)
    m = g.binop(synth.K_MUL, dl, synth.C(np.float32(0.5)), V)
    q = g.nodes(synth.K_DIV, V)
    g.edge(m, q, 0, 0)
    g.edge(0, q, 1, 1)
    r = g.binop(synth.K_MOD, q, synth.C(np.float32(1.5)), V)
    mn = g.binop(synth.K_MIN, r, v, V)
    g.edge(v, x, 0, 0)
    g.edge(mn, x, 0, 1)
    g.edge(x, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def bus_one_pole_tree(V, P, B_=2, a=0.25, b=0.75):
    """Voices x gain, voices k::B_ summed to bus k, each bus through y = a * bus + b * Delay(y, 1)."""
    g = synth.GraphArrays()
    bus = B._buses(g, B._gained_voices(g, V, P, False), B_)
    y = _loop(g, g.binop(synth.K_MUL, bus, synth.C(np.float32(a)), B_), [(1, b)], B_)
    g.edge(y, 0, 0, np.arange(B_, dtype=np.uint32))
    return g.finish(B_)


def summed_one_poles_tree(V, P):
    """Each voice through its own one-pole y_v = 0.5 * voice_v + 0.5 * Delay(y_v, 1), the V filters summed to one row."""
    g = synth.GraphArrays()
    y = _loop(g, g.binop(synth.K_MUL, _voices(g, V, P), synth.C(np.float32(0.5)), V), [(1, 0.5)], V)
    out = synth.sum_tree(g, np.asarray(y)[None, :])
    g.edge(out, 0, 0, 0)
    return g.finish(1)


def two_banks_tree(sizes=((1, 256), (2, 128)), d=3):
    """Voices of two sizes (two bank launches), each through comb(d)."""
    g = synth.GraphArrays()
    v = np.concatenate([_voices(g, V, P, 0x5EED0810 + P) for V, P in sizes])
    x = _loop(g, v, [(d, 0.6)], len(v))
    g.edge(x, 0, 0, np.arange(len(v), dtype=np.uint32))
    return g.finish(len(v))


def many_reads_tree(V, P, n):
    """x = voice + sum of n taps Delay(x, k + 1) * 2^-(k + 2): n own reads and the voice's ring: n + 1 loads."""
    g = synth.GraphArrays()
    x = _loop(g, _voices(g, V, P), [(k + 1, 2.0 ** -(k + 2)) for k in range(n)], V)
    g.edge(x, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def dyn_loop_tree(V, P):
    """x = voice + 0.5 * Delay(x, 1) + 0.25 * Delay(voice, 1 + 30 * Modulo(t * 0.001, 1)): a Delay by a signal amount (bounded:
    1..31 frames; of the voice: a feedback plan takes no signal Delay of a computed value) inside a one-sample loop's program."""
    g = synth.GraphArrays()
    f = np.float32
    v = _voices(g, V, P)
    lfo = g.binop(synth.K_MOD, g.binop(synth.K_MUL, synth.IN(0), synth.C(f(0.001)), 1), synth.C(f(1.0)), 1)
    amt = g.binop(synth.K_SUM2, synth.C(f(1.0)), g.binop(synth.K_MUL, synth.C(f(30.0)), lfo, 1), 1)
    x = g.nodes(synth.K_SUM2, V)
    d1 = g.nodes(synth.K_DELAY, V)
    g.const(d1, f(1.0), 1)
    d2 = g.nodes(synth.K_DELAY, V)
    g.edge(np.broadcast_to(amt, (V,)), d2, 0, 1)
    inner = g.binop(synth.K_SUM2, g.binop(synth.K_MUL, d1, synth.C(f(0.5)), V), g.binop(synth.K_MUL, d2, synth.C(f(0.25)), V), V)
    g.edge(v, x, 0, 0)
    g.edge(inner, x, 0, 1)
    g.edge(x, d1, 0, 0)
    g.edge(v, d2, 0, 0)
    g.edge(x, 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def ring_of_loops_tree(P, n):
    """x_0 = voice + 0.5 * Delay(x_(n-1), 1), x_i = 0.5 * Delay(x_(i-1), 1): n delay lines on ONE cycle, so the plan's one-launch
    form merges them into one program that stores n rings (and has n + 1 loads).  Row 0 = x_(n-1)."""
    g = synth.GraphArrays()
    v = _voices(g, 1, P)
    dl = g.nodes(synth.K_DELAY, n)
    g.const(dl, np.float32(1.0), 1)
    m = g.binop(synth.K_MUL, dl, synth.C(np.float32(0.5)), n)
    x0 = g.binop(synth.K_SUM2, v, m[:1], 1)
    x = np.concatenate([x0, m[1:]])
    g.edge(np.roll(x, 1), dl, 0, 0)
    g.edge(x[-1], 0, 0, 0)
    return g.finish(1)


def _case(name, build, n_rows, options, strides, per_voice, bus, delays, n_in=1, oracle_share=1):
    """strides: the nonzero entries of stream.loop_programs, sorted; per_voice / bus: programs_per_voice and bus_programs;
    delays: the loop's own taps (the oracle's cost model); oracle_share: rows that each re-evaluate the loop per frame."""
    return {"name": name, "build": build, "n_rows": n_rows, "options": options, "strides": strides, "per_voice": per_voice, "bus": bus,
            "oracle_frames": oracle_frames(delays, ORACLE_BUDGET // oracle_share), "n_in": n_in}


SERVABLE = [_case(f"comb_{d}_2x{P}", (lambda d=d, P=P: comb_tree(2, P, d)), 2, OPTION, [d, d], [1, 1], 0, (d,))
            for P in (128, 256) for d in (1, 5, 32, 63)] + [
    _case("taps_2_3", lambda: taps_tree(2, 128, (2, 3)), 2, OPTION, [1, 1], [1, 1], 0, (2, 3)),
    _case("taps_6_9", lambda: taps_tree(2, 128, (6, 9)), 2, OPTION, [3, 3], [1, 1], 0, (6, 9)),
    _case("taps_3_441", lambda: taps_tree(2, 128, (3, 441)), 2, OPTION, [3, 3], [1, 1], 0, (3, 441)),
    # per voice: the loop (it stores its ring and writes the row that is x itself) and the tap behind it
    _case("tap_behind_loop", lambda: tap_behind_tree(2, 128), 4, OPTION, [5, 5], [2, 2], 0, (5,), oracle_share=2),
    _case("arith_loop", lambda: arith_tree(2, 128), 2, INPUTS, [1, 1], [1, 1], 0, (1,), n_in=2),
    # 3 voices to 2 buses: bus 0 = two voices (a bus program), bus 1 = one voice alone (a program of that voice, whichever
    # number the bank gives it: programs_per_voice is compared sorted)
    _case("bus_one_pole_3x128_2", lambda: bus_one_pole_tree(3, 128), 2, BUS, [1, 1], [0, 0, 1], 1, (1,)),
    _case("bus_echo_32", lambda: B.bus_comb_tree(2, 128, 32), 1, BUS, [32], [0, 0], 1, (32,)),
    _case("summed_one_poles", lambda: summed_one_poles_tree(3, 128), 1, BUS, [1], [0, 0, 0], 1, (1,)),
    _case("two_banks_comb_3", lambda: two_banks_tree(), 3, BANKS, [3, 3, 3], [1, 1, 1], 0, (3,)),
]

# (name, builder, output rows, options, fragment of the reason with FR_STREAM_LOOPS on)
REFUSED = [
    ("too_many_loads", lambda: many_reads_tree(2, 128, LOOP_LOADS), 2, OPTION,
     f"a loop program has {LOOP_LOADS + 1} frame-only loads; block streaming serves at most {LOOP_LOADS}"),
    ("too_many_stores", lambda: ring_of_loops_tree(128, LOOP_STORES + 1), 1, OPTION,
     f"a loop program stores {LOOP_STORES + 1} rings; block streaming serves at most {LOOP_STORES}"),
    ("dyn_in_loop", lambda: dyn_loop_tree(2, 128), 2, OPTION, "S_READ_DYN (a Delay by a signal amount), which block streaming does not serve yet"),
]


def case(name):
    for c in SERVABLE:
        if c["name"] == name:
            return c
    raise KeyError(name)


def check_stream_object(s, c):
    """fr_plan_json["stream"] of a servable case against the graph's expectations."""
    assert s["servable"] is True and s["reason"] == "", s
    assert s["kernel"] == NEW_KERNEL, s
    assert sorted(l for l in s["loop_programs"] if l) == sorted(c["strides"]), s
    assert len(s["loop_programs"]) == sum(s["programs_per_voice"]) + s["bus_programs"], s
    assert sorted(s["programs_per_voice"]) == sorted(c["per_voice"]) and s["bus_programs"] == c["bus"], s
    assert s["loop_loads"] == LOOP_LOADS and s["loop_stores"] == LOOP_STORES, s


def blocks_of(rows, rng=None, n_in=1):
    """[(idx, T, [time row, control rows ...])] from stream_cases-style [(idx, row)]; control rows of every hostile kind."""
    out = []
    for k, (idx, t) in enumerate(rows):
        T = len(t)
        out.append((idx, T, [t] + [I.control_row(rng, T, 5 if k % 2 else 0) for _ in range(1, n_in)]))
    return out


def stream_all(lib, tree, n_rows, blocks, options, semantics="reference"):
    """The blocks through fr_stream_block_rows of a renderer with `options`; returns the blocks' results and the plan."""
    from libfriendship_amd.capi import Renderer
    with Renderer(lib, semantics=semantics, options=dict(options, **IDLE)) as s:
        synth.install(s, tree)
        s.stream_begin(n_rows)
        got = [s.stream_block_rows(idx, rows, n_times=T) for idx, T, rows in blocks]
        plan = s.plan()
        s.stream_end()
    return got, plan


def fill_compare(lib, tree, n_rows, blocks, got, what, semantics="reference", upto=None):
    """The same blocks through fr_fill_buffer of a renderer of `lib` with no option set (the first call is a seek); every
    sample equal bit for bit.  `upto`: only the frames before that one (the blocks are consecutive from 0; the block that
    crosses it is rendered and compared up to it).  Returns the frames compared."""
    from libfriendship_amd.capi import Renderer
    n = 0
    with Renderer(lib, semantics=semantics) as f:
        synth.install(f, tree)
        for k, ((idx, T, rows), a) in enumerate(zip(blocks, got)):
            if upto is not None:
                T = min(T, upto - idx)
                if T <= 0:
                    break
            b = f.fill_buffer(n_rows, idx, idx + T, [r[:T] for r in rows])
            assert K.same_bits(a[:, :T], b), f"block {k} at frame {idx} (T={T}) {what}: " + K.first_diff(a[:, :T], b)
            n += T
    return n
