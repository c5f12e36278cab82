"""The streaming matrix on the CPU (tests/stream_matrix.py): before anything runs on a GPU, the dense reference of
tests/stream_reference.py and the cases themselves are proven here.
  * the reference equals the simulator's fr_fill_buffer of the same blocks, no stream option set, bit for bit on every block
    (a fresh renderer per stream: its first call is a seek, as a stream's first block is);
  * on the first segment, up to the case's oracle budget, it equals the C++ oracle;
  * in every output row at least 95 % of the expected samples are finite -- a condition on the INPUTS: in x = voice + g * Delay(x, d)
    a NaN never leaves, and a comparison of NaN with NaN checks nothing;
  * raising every constant Delay amount by one frame changes at least 90 % of the finite samples of every row such a Delay feeds
    (arith_loop: 25 %, its Minimum and Modulo mask the delay): a kernel that reads one frame off cannot pass;
  * with the case's options fr_plan_json["stream"] is servable, shows the case's features and names the kernel where the plan
    alone decides it; the table as a whole holds every (kernel, inherited feature) pair and the all-features patch.
The last test measures the finite share of the older tests' sequences (stream_cases.block_rows), which is why the matrix exists:
profiles/stream_matrix.txt has the figures."""
import numpy as np
import pytest

import sim_tools
import stream_cases as K
import stream_loop_cases as L
import stream_matrix as X
import stream_reference as SR
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

NAMES = [c["name"] for c in X.CASES]
WRAPS = [c["name"] for c in X.WRAPS]


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in list(X.ALL) + ["FR_LOOP_TILES", "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"]:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("name", NAMES + WRAPS)
def test_the_reference_equals_the_simulator(sim, name):
    c = X.case(name)
    tree, streams, expected = X.reference_of(name)
    n = 0
    for s, (blocks, exp) in enumerate(zip(streams, expected)):
        with Renderer(sim, semantics=c["semantics"]) as f:
            synth.install(f, tree)
            for k, ((idx, T, rows), e) in enumerate(zip(blocks, exp)):
                got = f.fill_buffer(c["n_rows"], idx, idx + T, rows)
                assert not SR.first_diff(got, e, f"{name} stream {s} block {k} at frame {idx} (T={T}), fr_fill_buffer against the reference")
                n += T
    assert n == X.frames_of(c)
    if name in WRAPS:                                                  # the stream crosses the ring's end, and not as NaN
        idxs = [idx for idx, _, _ in streams[0]]
        assert streams[0][-1][0] + streams[0][-1][1] > X.RING_FRAMES
        share = SR.finite_share(expected[0], X.RING_FRAMES, idxs)
        print(f"{name}: finite beyond frame {X.RING_FRAMES}: {share}")
        assert (share >= X.FINITE_SHARE).all(), share


@pytest.mark.parametrize("name", NAMES + WRAPS[:1])
def test_the_reference_equals_the_oracle(oracle_lib, name):
    c = X.case(name)
    tree, streams, expected = X.reference_of(name)
    n = 0
    with Renderer(oracle_lib, semantics=c["semantics"]) as o:
        synth.install(o, tree)
        for k, ((idx, T, rows), e) in enumerate(zip(streams[0], expected[0])):
            T = min(T, c["oracle_frames"] - idx)
            if T <= 0:
                break
            got = o.fill_buffer(c["n_rows"], idx, idx + T, [r[:T] for r in rows])
            assert not SR.first_diff(got, e[:, :T], f"{name} block {k} at frame {idx} (T={T}), the oracle against the reference")
            n += T
    assert n == c["oracle_frames"] > 0


@pytest.mark.parametrize("name", NAMES)
def test_every_row_is_mostly_finite(name):
    _, _, expected = X.reference_of(name)
    share = SR.finite_share([a for exp in expected for a in exp])
    print(f"{name}: finite share per row {np.round(share, 4)}")
    assert (share >= X.FINITE_SHARE).all(), share
    assert max(float(np.abs(np.where(np.isfinite(a), a, 0)).max()) for exp in expected for a in exp) > 0.01


@pytest.mark.parametrize("name", [c["name"] for c in X.CASES if c["delay_rows"]])
def test_a_delay_one_frame_off_shows(name):
    c = X.case(name)
    tree, streams, expected = X.reference_of(name)
    assert SR.rows_behind_constant_delays(tree) == c["delay_rows"]
    first = [streams[0][k] for k in SR.segments_of(streams[0])[0]]       # the first segment's blocks
    ref = np.concatenate(expected[0][:len(first)], axis=1)
    off = np.concatenate(SR.expected_blocks(SR.with_delays_raised(tree), first, c["semantics"]), axis=1)
    past = int(SR.constant_delays(tree).max()) + 1
    assert past + 200 <= ref.shape[1]
    for r in c["delay_rows"]:
        a, b = ref[r, past:], off[r, past:]
        finite = np.isfinite(a)
        differ = (a.view(np.uint32) != b.view(np.uint32))[finite].mean()
        print(f"{name} row {r}: {differ:.4f} of {finite.sum()} finite samples differ with every constant delay one frame longer")
        assert differ >= c["sensitivity"], (r, differ)


@pytest.mark.parametrize("name", NAMES + WRAPS)
def test_the_serving_rule(sim, name):
    c = X.case(name)
    tree = c["build"]()
    with Renderer(sim, semantics=c["semantics"], options=c["options"]) as r:
        synth.install(r, tree)
        r.fill_buffer(c["n_rows"], 0, 64, [synth.time_ramp(0, 64)] + [np.ones(64, np.float32)] * (c["n_in"] - 1))
        plan = r.plan()
    s = plan["stream"]
    assert s["servable"] is True and s["reason"] == "", s
    if name in WRAPS:
        assert plan["feedback"] and s["kernel"] == X.KERNEL_NAME["loops"], s
        return
    assert X.features_of(s) == c["features"], (sorted(X.features_of(s)), s)
    assert bool(plan["feedback"]) == c["feedback"], plan["feedback"]
    top = max(c["features"], key=X.KERNELS.index) if c["features"] else "plain"
    assert c["kernel"] == top
    if c["kernel"] in X.BY_PLAN:
        assert s["kernel"] == X.KERNEL_NAME[c["kernel"]], s
    assert len(s["input_slots"]) == c["n_in"], s


def test_the_table_covers_the_cascade():
    have = {(c["kernel"], f) for c in X.CASES for f in c["features"] if f != c["kernel"]}
    assert len(X.PAIRS) == 21 and not [p for p in X.PAIRS if p not in have], [p for p in X.PAIRS if p not in have]
    assert {c["kernel"] for c in X.CASES} == set(X.KERNEL_NAME)
    assert X.case(X.ALL_FEATURES)["features"] == frozenset(X.KERNELS) and X.case(X.ALL_FEATURES)["kernel"] == "dyn"
    assert {c["name"] for c in L.SERVABLE} <= set(NAMES)
    sparkle = {c["kernel"] for c in X.CASES if c["semantics"] == "sparkle"}
    assert {"loops", "dyn"} <= sparkle and X.case(X.ALL_FEATURES + "_sparkle")["semantics"] == "sparkle"
    for c in X.CASES:
        assert 1350 <= X.frames_of(c) <= 1950 and 0 < c["oracle_frames"] <= c["streams"][0][0][1]
        assert X.frames_beyond_oracle(c) >= 650                          # the seeks and the second stream, at the least
        assert X.poisoned_frames(c) <= X.POISONED_SHARE * X.frames_of(c) and X.POISONED_SHARE < 1 - X.FINITE_SHARE
        assert [[b[1] for b in blocks[:7]] for blocks in X.streams_of(c)][0] == list(K.FIRST_LENGTHS)


# ---- why the matrix exists: the older device tests' sequences (stream_cases.block_rows) behind feedback --------------------------
# (id, builder, input rows, seed, starts, knob): the sequences of tests/test_hip_stream_{loops,general,dyn,programs,bus}.py, rebuilt
# as those tests build them.  Whether a sample of a comb is finite depends on the time rows and the loop alone, not on the voices'
# size or number, so the sequences of 33 500 frames and more are measured on one voice of 128 partials with the same loop.

def _old_loops(name):
    c = L.case(name)
    return (f"loops/{name}", c["build"], c["n_in"], len(name) * 7919, [(0, 1500)], False)


# Not listed: arith_loop, whose Minimum drops a NaN operand (99.1 % finite), and the comb(64) of test_jumps_forward_and_back_are_seeks,
# whose segments are too short for the poison to spread (97.1 %).
OLD = [_old_loops(c["name"]) for c in L.SERVABLE if c["name"] != "arith_loop"] + [
    ("general/comb_5_2x100", lambda: K.comb_tree(2, 100, 5), 1, len("comb_5_2x100") * 7919, [(0, 1500)], False),
    ("dyn/beside_loop", X.case("beside_loop")["build"], 1, len("beside_loop") * 7919, [(0, 1500)], False),
    ("loops/test_the_rings_wrap", lambda: K.comb_tree(1, 128, 5), 1, 5, [(0, 33500)], False),
    ("loops/test_jumps_are_seeks[1]", lambda: K.comb_tree(2, 128, 1), 1, 1, [(0, 300), (9000, 200), (2500, 200), (40000, 100), (64, 100)], False),
    ("loops/test_jumps_are_seeks[5]", lambda: K.comb_tree(2, 128, 5), 1, 5, [(0, 300), (9000, 200), (2500, 200), (40000, 100), (64, 100)], False),
    ("programs/comb_64 from 130", lambda: K.comb_tree(1, 128, 64), 1, len("comb_64") * 7919 + 2, [(130, 33500)], False),
    ("programs/comb_441 from 500", lambda: K.comb_tree(1, 128, 441), 1, 16, [(500, 34000)], False),
    ("bus/bus_comb_64 from 130", lambda: X.B.bus_comb_tree(2, 128, 64), 1, len("bus_comb_64") * 7919 + 2, [(130, 33500)], False),
]


@pytest.mark.parametrize("old", OLD, ids=[o[0] for o in OLD])
def test_the_older_sequences_compare_nan_with_nan(old):
    """Measured, and asserted only as far as it is the reason for the matrix: behind feedback the older sequences are less than
    95 % finite (most of them far less), so beyond the first poisoned block they compare NaN with NaN."""
    name, build, n_in, seed, starts, _ = old
    rng = np.random.default_rng(seed)
    blocks = L.blocks_of(K.block_rows(rng, starts), rng, n_in)
    exp = SR.expected_blocks(build(), blocks)
    share = SR.finite_share(exp)
    a = np.concatenate(exp, axis=1)
    whole = np.isfinite(a).all(axis=0)
    tail = int(np.nonzero(whole)[0][-1]) if whole.any() else -1            # the last column (in stream order) with every row finite
    at = np.concatenate([np.arange(idx, idx + T) for idx, T, _ in blocks])
    print(f"OLD {name}: frames {a.shape[1]}, finite {100 * share.min():.1f} %, last finite frame in stream order {int(at[tail])} (sample {tail})")
    assert share.min() < X.FINITE_SHARE
