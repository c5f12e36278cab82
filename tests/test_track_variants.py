"""Track voices on the CPU: the dense per-frame reference (bank_reference.render_track_bank) pinned bit for bit to the C++
oracle, which gets the rows as ordinary inputs, on the values where kernels go wrong and under the reference's dropped-row
quirk; the GPU case table (tests/track_variants.py) checked against every key the launch rule can produce for a group with
tracks (tests/cpp/bankplan_sweep.cpp --tracks, --query); the conditions the GPU test's matrices must meet; and the ring-span
sequences' expectation -- the dense reference over absolute frames, shifted by the delay -- against the oracle."""
import subprocess

import numpy as np
import pytest

import bank_reference
import sim_tools
import track_rows
import track_variants
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_UNSUPPORTED, RenderError, Renderer
from test_bank_variants import HOSTILE, _sweep_bin, query

_F = np.float32


# ---- the dense reference against the C++ oracle ---------------------------------------------------------------------------
def _hostile_tracks(V, P, idx, T, seed):
    """Regular rows, then per voice: 0 hostile w values (negative, -0, NaN, +-inf, 1e30, subnormals, t * w integral or beyond
    2^23) cycling over partials and frames; 1 hostile amplitudes (+0, -0, negatives, NaN, inf, subnormal); 2 every row -0;
    3 negative w rows; 4 amplitudes of mixed +0 / -0 under sounding w; 5 regular."""
    m = track_rows.regular_rows(V, P, idx, T, seed)
    k, f = np.arange(P)[:, None], np.arange(T)[None, :]
    wrow = lambda v: m[1 + 2 * v * P:1 + 2 * (v + 1) * P:2]
    arow = lambda v: m[2 + 2 * v * P:2 + 2 * (v + 1) * P:2]
    wrow(0)[:] = track_rows.HOSTILE_W[(k + 3 * f) % len(track_rows.HOSTILE_W)]
    arow(1)[:] = track_rows.HOSTILE_AMP[(5 * k + f) % len(track_rows.HOSTILE_AMP)]
    wrow(2)[:] = -0.0
    arow(2)[:] = -0.0
    wrow(3)[:] *= _F(-1.0)
    arow(4)[:] = np.where((k + f) % 2 == 0, _F(0.0), _F(-0.0))
    return m


@pytest.mark.parametrize("P", [1, 3, 8, 24, 256])
def test_track_reference_matches_oracle(oracle_lib, P):
    """Every frame, bit for bit.  A priming call that makes every row live, then: a ramp at a large offset over regular rows;
    the hostile time values over regular rows; hostile track rows under the ramp, and under the hostile time values."""
    V = 6
    tree = synth.track_tree(V, P)
    T = 40
    assert len(HOSTILE) <= T
    pad = lambda row: np.concatenate([row, np.arange(len(row), T, dtype=_F)])
    with Renderer(oracle_lib) as ref:
        synth.install(ref, tree)
        limit = track_rows.SlotLimit()
        idx = track_rows.OFFSET
        calls = [("priming", track_rows.priming_slots(V, P, T), track_rows.regular_rows(V, P, idx, T, P))]
        m = track_rows.regular_rows(V, P, idx + T, T, P + 1)
        m[0] = pad(HOSTILE)
        calls.append(("hostile time", V, m))
        calls.append(("hostile tracks", V, _hostile_tracks(V, P, idx + 2 * T, T, P + 2)))
        m = _hostile_tracks(V, P, idx + 3 * T, T, P + 3)
        m[0] = pad(HOSTILE)
        calls.append(("hostile tracks and time", V, m))
        m = track_rows.regular_rows(V, P, idx + 4 * T, T, P + 4)
        m[0] = -np.arange(0, T, dtype=_F) * _F(0.37)
        calls.append(("negative ramp", V, m))
        for what, n_slots, m in calls:
            assert m.shape == (tree["n_inputs"], T)
            lim = limit.call(n_slots, T)
            assert lim >= tree["n_inputs"], what
            exp = ref.fill_buffer_dense(n_slots, idx, idx + T, m)
            w, amp = bank_reference.track_params(m, V, P, lim)
            got = bank_reference.render_track_bank(w, amp, m[0], budget=1 << 12)
            msg = bank_reference.first_diff(got, exp[:V], f"P={P} {what}")
            assert not msg, msg
            assert not exp[V:].any()
            # voices and frames cut into many slices give the same bits as one slice
            assert not bank_reference.first_diff(bank_reference.render_track_bank(w, amp, m[0], budget=P * 7), got)
            idx += T
        assert track_rows.quiet_voices_sound(exp[:V], hostile=()) == "", "the regular rows do not sound"


def test_constant_rows_give_the_constant_bank():
    """Rows that hold one value per partial render as render_bank's constants do: the per-frame path is the same operations."""
    rng = np.random.default_rng(3)
    w = (rng.random((3, 24)) * 0.05 - 0.01).astype(_F)
    amp = rng.normal(size=(3, 24)).astype(_F)
    t = np.concatenate([HOSTILE, np.arange(1 << 20, (1 << 20) + 50, dtype=_F)])
    T = len(t)
    got = bank_reference.render_track_bank(np.repeat(w[:, :, None], T, 2), np.repeat(amp[:, :, None], T, 2), t)
    assert not bank_reference.first_diff(got, bank_reference.render_bank(w, amp, t))


# (n_slots, frames) of a first call on a fresh renderer of 2 voices x 16 partials (65 rows), and the first slot it drops
@pytest.mark.parametrize("n_slots,T,what", [(2, 7, "between partial 6's w slot 13 and its amp slot 14"),
                                            (3, 7, "at partial 10's w slot 21, inside the group of partials 8 .. 15")])
def test_dropped_rows_match_the_oracle(oracle_lib, n_slots, T, what):
    """The reference keeps n_slots * n_times input vectors of the largest call so far and drops the rows beyond them: a fresh
    oracle, a short first call, a shorter one (the limit stays), a longer one (it grows), one that makes every row live."""
    V, P = 2, 16
    tree = synth.track_tree(V, P)
    limit = track_rows.SlotLimit()
    limits = []
    with Renderer(oracle_lib) as ref:
        synth.install(ref, tree)
        idx = 0
        for k, (ns, n) in enumerate([(n_slots, T), (2, 5), (2, 9), (2, 40)]):
            m = track_rows.span_rows(V, P, idx, n, 100 + k)
            lim = limit.call(ns, n)
            limits.append(lim)
            if lim < tree["n_inputs"]:
                # a partial whose amp slot is dropped is 0 * parab(t * w) whatever its w row holds, unless that is not finite:
                # an infinite w at one frame of the w row at the limit (the last live slot, or the first dropped one) makes
                # that row show, as 0 * NaN, exactly when it is live
                m[lim - 1 if lim % 2 == 0 else lim, n // 2] = np.inf
            exp = ref.fill_buffer_dense(ns, idx, idx + n, m)
            got = track_rows.expected(V, P, m, lim)
            msg = bank_reference.first_diff(got, exp[:V], f"{what}: call {k}, limit {lim}")
            assert not msg, msg
            for off in (-1, 1):   # (the test can tell: one slot either way gives other bits while the limit cuts the rows)
                if lim < tree["n_inputs"]:
                    assert bank_reference.first_diff(track_rows.expected(V, P, m, lim + off), exp[:V]), (what, k, off)
            idx += n
    assert limits == [n_slots * T, n_slots * T, 18 if n_slots == 2 else 21, 80]
    first_dropped = n_slots * T
    assert (first_dropped - 1) % 2 == (1 if n_slots == 2 else 0)      # an amp slot / a w slot
    assert ((first_dropped - 1) // 2) % 8 not in (0,) and (first_dropped - 1) // 2 < P


# ---- the launch rule's reachable forms for groups with tracks -----------------------------------------------------------
def case_launch(case, n_times):
    """The bankplan_sweep --query line of a case's call: a compiled group with tracks whose module has the whole-voices entry."""
    o = case["options"]
    fields = [1, case["P"].bit_length() - 1, case["V"], 0, 1, 1, n_times, 0, 0, 1, 1000, 0, 0, 0, 0, int(o.get("FR_BANK_MULTI", "1") != "0"), 1,
              int(o.get("FR_JIT_CHUNKS", "1") != "0"), o.get("FR_JIT_CHUNK_TARGET", 0)]
    return " ".join(str(f) for f in fields)


def test_table_has_exactly_the_reachable_keys():
    """bankplan_sweep --tracks: the keys the rule can produce for a group with tracks are the table's keys."""
    p = subprocess.run([_sweep_bin(), "--tracks"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    reached = {ln.split("\t")[0] for ln in lines[:-1]}
    assert lines[-1].startswith(f"{len(reached)} keys"), lines[-1]
    assert all("tracks=1" in ln for ln in lines[:-1])
    table = {c["key"] for c in track_variants.CASES}
    assert reached == table, (sorted(reached - table), sorted(table - reached))
    assert not reached & set(track_variants.UNREACHABLE)
    names = [c["name"] for c in track_variants.CASES]
    assert len(names) == len(set(names))


def test_every_case_reaches_its_key():
    """Each case reaches its key on both call lengths, its first call's workgroup count is a multiple of 8 exactly where the
    table says so, its shape can hold the hostile placements, and the table covers what the issue of a track kernel needs:
    every entry point, both sides of the XCD remap, the reload of the next group's rows and its absence, the short-call rule
    with the piece count it gives, and the priming call's arithmetic."""
    cases = track_variants.CASES
    got = query([case_launch(c, T) for c in cases for T in (c["T"], c["T2"])])
    for i, c in enumerate(cases):
        (k1, n1, vpw), (k2, _, _) = got[2 * i], got[2 * i + 1]
        assert k1 == c["key"] and k2 == c["key"], (c, k1, k2)
        assert (n1 % 8 == 0) == c["xcd"], (c["name"], n1)
        assert c["T"] % 64 and c["T2"] % 64 and c["T"] != c["T2"] and c["T"] > 64 + 24, c
        assert c["V"] >= 3 and c["P"] >= 32, c
        assert (vpw != 0) == (c["key"] == "jit_bank_multi"), c
        if vpw:
            assert c["V"] % (4 * vpw), c
        assert c["groups"] >= 1 and c["groups"] * 8 * (1 if vpw else 4) << c["pieces_log2"] == c["P"], c
        assert track_rows.priming_slots(c["V"], c["P"], c["T"]) * c["T"] >= 1 + 2 * c["V"] * c["P"]
    assert {c["entry"] for c in cases} == {"dense", "csr", "device_dense"}
    for fam in track_variants.XCD_FAMILIES:
        assert {c["xcd"] for c in cases if c["key"].startswith(fam)} == {True, False}, fam
    for k in range(1, 7):   # every piece count with the reload: two groups per wave and more
        assert any(c["pieces_log2"] == k and c["groups"] >= 2 for c in cases), k
    assert any(c["groups"] == 1 for c in cases)
    # the n_times <= 128 && log2_p >= 8 rule: pieces of 256 partials, where the target alone gives another count
    rule = [c for c in cases if c["T"] <= 128 and c["T2"] <= 128 and c["P"] >= 256 and "FR_JIT_CHUNK_TARGET" not in c["options"]]
    assert {c["P"] >> c["pieces_log2"] for c in rule} == {256} and {c["pieces_log2"] for c in rule} >= {0, 2}, rule
    for c in rule:
        (k129, _, _), = query([case_launch(c, 129)])
        assert k129 != c["key"], (c, k129)
    default = [c for c in cases if not c["options"] and c["T"] > 128]
    assert default, "no case under the default target"
    # the default target itself, 16384 workgroups for tracks, binds only at sizes no test should carry: pinned here from the
    # rule at the benchmark's shape, 64 voices x 4096 partials (16 pieces at 64 and at 1024 frames, 4 at 4800)
    bench = {"V": 64, "P": 4096, "options": {}}
    assert [k for k, _, _ in query([case_launch(bench, T) for T in (64, 1024, 4800)])] == ["jit_bank/pieces4", "jit_bank/pieces4", "jit_bank/pieces2"]
    fresh = [c for c in cases if c["fresh"]]
    assert len(fresh) == 1
    c = fresh[0]
    dropped = c["V"] * c["T"]                     # the first slot the un-primed renderer drops
    leaf = (dropped - 1) // 2
    assert dropped < 1 + 2 * c["V"] * c["P"] and (dropped - 1) % 2 == 1, "the limit falls between a partial's w and its amp"
    assert 0 < leaf % c["P"] < c["P"] - 1 and leaf % 8 not in (0, 7), "mid-voice and mid-group"


@pytest.mark.parametrize("case", track_variants.CASES, ids=[c["name"] for c in track_variants.CASES])
def test_gpu_matrices_meet_their_conditions(case):
    """What tests/test_hip_track_matrix.py asserts on the reference, checked here for the very matrices it uses: hostile values
    touch two voices and five frames at the most, and every other voice is finite and nonzero in at least half its samples --
    in the regular calls every voice."""
    V, P, T = case["V"], case["P"], case["T"]
    seed = P * 7 + V
    m, hostile = track_rows.hostile_rows(case, track_rows.OFFSET + T, seed)
    reg = track_rows.regular_rows(V, P, track_rows.OFFSET + T, T, seed)
    changed = np.argwhere(m[1:].view(np.uint32) != reg[1:].view(np.uint32))
    assert len(changed)
    assert set(np.unique(changed[:, 0] // (2 * P))) <= set(hostile) and len(hostile) <= 2
    assert set(np.unique(changed[:, 1])) <= set(track_rows.hostile_frames(T)) and len(track_rows.hostile_frames(T)) <= 5
    assert {63, 64, T - 1} <= set(np.unique(changed[:, 1]))
    leaves = {int(s) // 2 % P for s in np.unique(changed[changed[:, 0] // (2 * P) == 0][:, 0])}
    piece = P >> case["pieces_log2"]
    assert {0, 7, P - 8, P - 1} <= leaves
    if case["pieces_log2"]:
        assert {piece - 8, piece - 1} <= leaves and piece < P
    assert not np.isfinite(m[1:]).all() and (m[1:] == 0).any() and (m[1::2] < 0).any()
    assert track_rows.quiet_voices_sound(track_rows.expected(V, P, m), hostile) == ""
    assert track_rows.quiet_voices_sound(track_rows.expected(V, P, reg)) == ""
    if case["fresh"]:
        assert track_rows.quiet_voices_sound(track_rows.expected(V, P, reg, V * T)[:1]) == ""


# ---- ring spans ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", track_variants.SPAN_CASES, ids=[c["name"] for c in track_variants.SPAN_CASES])
def test_span_sequences(oracle_lib, case):
    """The table's launch counts follow from the rules; each table sequence holds what its name says; and the expectation of
    the GPU test -- the dense reference over absolute frames, shifted by d -- equals the oracle on every sample."""
    V, P, d, H = track_variants.SPAN_V, track_variants.SPAN_P, case["d"], case["H"]
    assert 1 <= d <= H <= 64
    head, cap = 0, 0
    for idx, n, launches in case["calls"]:
        frames, cap = track_rows.span_launches(idx, n, d, head, cap)
        assert len(frames) == launches and frames[-1] == n and sum(frames) - n in (0, min(d, idx)), (case["name"], idx, n, frames)
        head = idx + n
    tree = track_rows.span_tree(V, P, d)
    dense = track_rows.SpanReference(V, P, d)
    with Renderer(oracle_lib) as ref:
        synth.install(ref, tree)
        for k, (idx, n, _) in enumerate(case["calls"]):
            m = track_rows.span_rows(V, P, idx, n, 7 + k)
            exp = ref.fill_buffer_dense(V, idx, idx + n, m)
            got = dense.call(idx, m)
            msg = bank_reference.first_diff(got, exp, f"{case['name']}: call {k} at {idx}")
            assert not msg, msg
            assert track_rows.quiet_voices_sound(got[:, d:]) == ""
    assert case["calls"][0][0] == 0 and V * case["calls"][0][1] >= tree["n_inputs"], "the first call primes every row"


def test_span_table_covers_the_wrap():
    """A window [idx - d, idx) that straddles a multiple of the history ring's capacity (two spans), one that starts exactly on
    it, the smallest history, a seek."""
    starts = []
    for c in track_variants.SPAN_CASES:
        head = 0
        for idx, n, launches in c["calls"]:
            if launches > 1:
                starts.append(((idx - c["d"]) & 63, launches, idx != head))
            head = idx + n
    assert any(pos + 40 > 64 and pos and launches == 3 for pos, launches, _ in starts)
    assert any(pos == 0 and launches == 2 for pos, launches, _ in starts)
    assert any(seek for _, _, seek in starts)
    assert min(c["H"] for c in track_variants.SPAN_CASES) == 1


@pytest.mark.parametrize("case", track_variants.SPAN_CASES, ids=[c["name"] for c in track_variants.SPAN_CASES])
def test_span_sequences_on_the_simulator(oracle_lib, case):
    """The host-logic simulator has no run-time compiler, so it renders these voices as stage programs that read the tracks
    through the history's window (engine.cpp prepare_tracks: the frames before idx gathered from the 64-frame ring across its
    wrap) -- not the span launches of a track voice, which only the GPU test runs, but the same sequences through the same
    input store, slot limit, ring growth and tail append: against the oracle and the dense reference, bit for bit."""
    V, P, d = track_variants.SPAN_V, track_variants.SPAN_P, case["d"]
    tree = track_rows.span_tree(V, P, d)
    dense = track_rows.SpanReference(V, P, d)
    with Renderer(sim_tools.sim_lib(), options={"FR_TRACK_HISTORY": str(case["H"])}) as sim, Renderer(oracle_lib) as ref:
        sim.set_track_inputs(1)
        synth.install(sim, tree)
        synth.install(ref, tree)
        for k, (idx, n, _) in enumerate(case["calls"]):
            m = track_rows.span_rows(V, P, idx, n, 7 + k)
            got = sim.fill_buffer_dense(V, idx, idx + n, m)
            msg = bank_reference.first_diff(got, ref.fill_buffer_dense(V, idx, idx + n, m), f"{case['name']}: call {k} at {idx}, oracle")
            assert not msg, msg
            msg = bank_reference.first_diff(got, dense.call(idx, m), f"{case['name']}: call {k} at {idx}, dense reference")
            assert not msg, msg
            plan = sim.plan()
            assert plan["banks"] == [] and plan["pull_rows"] == 0 and plan["track_lookback"] == d, plan
            assert plan["track_tail_launches"] == 1 and plan["track_history"] == case["H"], plan
