"""The absolute sample index at 2^24 .. 2^62 on the CPU (tests/abs_index.py): before anything runs on a GPU, the table and
the shift rule it rests on are proven here.
  * the table: the bases, what rebase() moves and what it leaves, where the sequence crosses B, which recipes it reuses;
  * in every case at least half of the expected samples of every output row are finite and non-zero (on the reference alone),
    and every row of a graph case follows its input rows;
  * the case's look-back, from fr_plan_json, fits below its seek point (the rule's precondition), and is above 100 frames
    exactly where the table says so -- in at least one case of every family;
  * THE SHIFT RULE, per case and base: the dense reference of the low twin equals the C++ oracle rendered at the high frames.
    Graphs of a few nodes: every sample at every base.  Patches with voices (the oracle walks every partial per sample): every
    sample at 2^32, and at the other bases output row 0 whole and all rows at abs_index.special_frames -- the first and last
    frame of each call, B - 1, B, B + 1, B + d.  oracle/ref_numpy.py allocates idx floats per input slot, so it can represent
    2^24 only (64 MB a slot): it renders the graph cases of at most three slots there;
  * the host-logic simulator (engine.cpp's own windows, floors, store and seek rule, plain-loop kernels) equals the
    expectation on every sample of every case at every base; a stream case through its fr_fill_buffer twin, a fresh
    renderer per stream, as in tests/test_stream_matrix.py (the simulator launches no resident kernel);
  * a feedback plan refuses a seek beyond 2^28 frames by name and serves the next seek to a low frame."""
import numpy as np
import pytest

import abs_index as A
import sim_tools
import stage_reference as sr
import stage_variants as sv
import stream_matrix as X

NAMES = [c["name"] for c in A.CASES]
FULL_ORACLE_BASE = 1 << 32
NUMPY_BASES = [1 << 24]


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in list(X.ALL) + ["FR_LOOP_TILES", "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"]:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_the_table_is_well_formed():
    assert A.BASES == [1 << 24, 1 << 31, 1 << 32, 1 << 40, 1 << 62]
    assert sorted(A.EVERY_CASE + A.PER_FAMILY) == A.BASES
    assert len(NAMES) == len(set(NAMES))
    # the stage forms: every feed-forward case of stage_variants that is not `wide`, keys as they are
    keys = [c["key"] for c in sv.CASES if c["seek"] is None and c["graph"][0] != "wide"]
    stages = [n for n in NAMES if n.startswith("stage:")]
    assert ["stage:" + k for k in keys] == stages[:18] and len(keys) == 18
    assert stages[18:] == ["stage:step/interpreter", "stage:step/compiled"]      # a Delay of a constant (S_STEP), which no case above has
    for flag in ("levels", "fused", "strided", "+table", "#dyn", "-sparkle", "stage_kernel/", "jit_stage[plain", "jit_stage[deep"):
        assert any(flag in k for k in keys), flag
    # the streams: every feed-forward case of the streaming matrix, every resident kernel that serves one
    ff = [c["name"] for c in X.CASES if not c["feedback"]]
    streams = [n for n in NAMES if n.startswith("stream:")]
    assert ["stream:" + n for n in ff] == streams[:23] and len(ff) == 23
    # ... and one case each of the later streaming modules: input history, short taps, patches without a voice, leaf programs
    assert streams[23:] == ["stream:eight_slots", "stream:env_taps_2x512", "stream:fir", "stream:tri_128", "stream:store_tap_150", "stream:trk_128"]
    assert {"observed:affine", "ring_keep:chains", "tracks:dense", "tracks:history", "bank:short", "bank:long", "bank:compiled", "pull:randgraph"} <= set(NAMES)
    assert {c["kernel"] for c in X.CASES if not c["feedback"]} == {"plain", "prog", "bus", "in", "banks", "general", "dyn"}
    for fam in A.FAMILIES:
        assert any(c["family"] == fam and c["deep"] for c in A.CASES), fam
        assert A.case(A.FAMILY_CASE[fam])["family"] == fam and A.case(A.FAMILY_CASE[fam])["deep"]
    assert {c["family"] for c in A.CASES} == set(A.FAMILIES) | {"tracks"}


@pytest.mark.parametrize("B", A.BASES)
def test_rebase_moves_the_index_and_nothing_else(B):
    for name in ("stage:stage_kernel/strided", "stream:taps_64_2x128"):
        c = A.case(name)
        low, _ = A.low_twin(name)
        high = A.rebase(low, B, c["s0"])
        far = [k for k, (idx, _, _) in enumerate(low) if idx - c["s0"] >= A.FAR_LOW]
        assert far and far == list(range(far[0], len(low)))                       # the far segment is the tail
        assert len(high) == (len(low) if B <= A.FAR_MAX_BASE else far[0])
        for k, ((li, lT, lrows), (hi, hT, hrows)) in enumerate(zip(low, high)):
            assert hT == lT and all(a is b for a, b in zip(lrows, hrows))          # the rows: the same arrays
            assert hi - B == (li - c["s0"] if k < far[0] else li - c["s0"] - A.FAR_LOW + A.FAR), k
        offs = [(idx - B, T) for idx, T, _ in high]
        assert offs[0][0] == A.SEEK and offs[1][0] == A.SEEK + offs[0][1]           # seek to B - 100, then contiguous
        crossing = [(o, T) for o, T in offs[:far[0]] if o < 0 < o + T - 1]
        assert len(crossing) == 2 and all(-o % 64 for o, _ in crossing)             # B inside a call, off the 64-frame groups
        assert (A.FORWARD in [o for o, _ in offs]) and (A.BACK in [o for o, _ in offs]) and any(T == 1 for _, T in offs)
        if B <= A.FAR_MAX_BASE:
            assert offs[far[0]][0] == (1 << 33) + 69
        # a time row follows the low ramp, never the moved index
        if name.startswith("stream:"):
            t = high[1][2][0]
            assert float(t[0]) == A.TIME0 + A.SEEK + 64 and float(t[0]) < 1 << 16


@pytest.mark.parametrize("name", NAMES)
def test_every_row_is_mostly_finite_and_non_zero(name):
    _, expected = A.low_twin(name)
    share = A.nonzero_share(expected)
    print(f"{name}: finite non-zero share per row {np.round(share, 3)}")
    assert (share >= A.NONZERO_SHARE).all(), share


@pytest.mark.parametrize("name", [c["name"] for c in A.CASES if c["s0"] == A.S0])
def test_every_row_follows_the_inputs(name):
    """With other values in every input row (other amounts in a Delay amount's row too), at least half of every expected row
    changes: a kernel that read +0 for an input, or another frame's value, could not pass.  (Rows of voices follow their time
    row by construction; a random graph may render constants, which the first choice of the pull case's seed did.)"""
    c = A.case(name)
    low, expected = A.low_twin(name)
    rng = np.random.default_rng(5)
    other = [(idx, T, [(np.where(np.isfinite(r), r, 0) * np.float32(0.75) + rng.normal(size=T)).astype(np.float32) for r in rows]) for idx, T, rows in low]
    a, b = np.concatenate(expected, axis=1), np.concatenate(c["expected"](other), axis=1)
    changed = (a.view(np.uint32) != b.view(np.uint32)).mean(axis=1)
    print(f"{name}: share of samples that follow the inputs, per row {np.round(changed, 3)}")
    if "#dyn" in name:       # row 2 of dyn_delays is Delay(3.5, in1): the constant wherever the amount is a number below 2^64, by construction
        changed = np.delete(changed, 2)
    assert (changed >= 0.5).all(), changed


def compare(name, what, got, expected):
    assert len(got) == len(expected) or what
    for k, (g, e) in enumerate(zip(got, expected)):
        msg = sr.first_diff(g, e, f"{name} {what}, call {k}")
        assert not msg, msg


def sim_twin(c):
    """The case as the simulator runs it: a stream case's blocks go through fr_fill_buffer, no stream option set."""
    return dict(c, entry="host", options={}) if c["kind"] == "stream" else c


def run_twin(lib, c, calls, options, after=None):
    """The sequence on `lib` through fr_fill_buffer (a mixed case: its script with every stream as its fr_fill_buffer twin)."""
    if c["kind"] == "mixed":
        return A.run_mixed(lib, c, calls, streamed=False, options=options, after=after)
    return A.run_calls(lib, dict(sim_twin(c), options=options), calls, after=after)


@pytest.mark.parametrize("name", NAMES)
def test_the_lookback_fits_below_the_seek_point(sim, name):
    c = A.case(name)
    low, expected = A.low_twin(name)
    plans = []
    got = run_twin(sim, c, low, c["options"], after=lambda p, k, T: plans.append(p))
    compare(name, "low twin on the simulator", got, expected)
    look = max(max(p.get("max_lookback", 0), p.get("stream", {}).get("lookback", 0), p.get("stream", {}).get("input_lookback", 0)) for p in plans)
    if c["mode"] == "pull":           # a Delay by a node's value has no bound the planner could show: the constants' amounts, from the graph
        look = sum(c["delays"])
        assert plans[0]["pull_rows"] == c["n_rows"]
    print(f"{name}: look-back {look}")
    assert look <= c["s0"] + A.SEEK, (look, c["s0"])
    assert (look > 100) == c["deep"], look
    if c["lookback"] is not None:
        assert look == c["lookback"], (look, c["lookback"])


@pytest.mark.parametrize("B", A.BASES)
@pytest.mark.parametrize("name", NAMES)
def test_the_shift_rule_against_the_oracle(oracle_lib, name, B):
    c = A.case(name)
    low, expected = A.low_twin(name)
    high = A.rebase(low, B, c["s0"])
    if c["s0"] == A.S0 or B == FULL_ORACLE_BASE:
        got = run_twin(oracle_lib, dict(c, mode="auto"), high, None)
        compare(name, f"oracle at {B}", got, expected)
        return
    frames = A.special_frames(high, B, c["delays"])
    assert {(k, idx) for k, (idx, T, _) in enumerate(high) for idx in (0, T - 1)} <= set(frames)
    assert sum(1 for k, col in frames if high[k][0] + col in (B - 1, B, B + 1)) >= 6      # the first segment and the seek back
    row0 = []
    at = A.oracle_at(oracle_lib, c, high, frames, row0)
    compare(name, f"oracle at {B}, row 0", row0, [e[:1] for e in expected])
    for (k, col), v in at.items():
        msg = sr.first_diff(v.reshape(-1, 1), expected[k][:, col:col + 1], f"{name}: oracle at frame {high[k][0] + col} (call {k})")
        assert not msg, msg


@pytest.mark.parametrize("B", NUMPY_BASES)
@pytest.mark.parametrize("name", [c["name"] for c in A.CASES if c["s0"] == A.S0 and c["n_in"] <= 3])
def test_the_shift_rule_against_ref_numpy(name, B):
    from oracle.ref_numpy import NumpyRefRenderer
    c = A.case(name)
    low, expected = A.low_twin(name)
    high = A.rebase(low, B, c["s0"])[:4]                                 # the segment that crosses B (a seek allocates idx floats again)
    r = NumpyRefRenderer(c["semantics"])
    c["install"](r)
    got = [r.fill_buffer(c["n_rows"], idx, idx + T, rows) for idx, T, rows in high]
    compare(name, f"ref_numpy at {B}", got, expected[:4])


@pytest.mark.parametrize("B", A.BASES)
@pytest.mark.parametrize("name", NAMES)
def test_the_simulator_at_the_high_index(sim, name, B):
    c = A.case(name)
    low, expected = A.low_twin(name)
    got = run_twin(sim, c, A.rebase(low, B, c["s0"]), sim_twin(c)["options"])
    compare(name, f"simulator at {B}", got, expected)


def test_a_feedback_plan_refuses_what_it_cannot_replay(sim):
    """A loop's state at frame 2^28 + 1 would take replaying 2^28 + 1 frames from 0 (csrc/callplan.hpp FB_MAX_REPLAY): refused
    with the frame's number, and the renderer serves the next seek to a low frame.  (Not sought: a seek to 2^28 itself, which is
    served -- by replaying 2^28 frames.)"""
    A.feedback_refusal(sim)
