"""Every launch form of a track voice (tests/track_variants.py), on the MI355X, against the dense per-frame f32 reference
(bank_reference.render_track_bank) on EVERY output sample, bit for bit (NaN == NaN).

Per case: the renderer gets the case's options and synth.track_tree(V, P) with its rows declared tracks, and each call asserts
from fr_plan_json the variant that ran and its pieces_log2, one bank launch over all V voices, `tracks` true, no pull rows, and
on the ramp the workgroup count against `xcd`.  Calls: a priming call that requests enough output slots to make every row live
(n_slots * T >= rows); a ramp at 2^20 + 37 of T frames (no multiple of 64); a hostile call of T frames (track_rows.hostile_rows:
hostile w / amp values in one voice's first and last group and in the last group of an inner piece, in one wave's share of
another voice, at frames 0, 63, 64, T / 2 and T - 1, under the hostile time row); a call of T2 frames that reuses the pieces'
workspace.  The `fresh` case runs again without the priming call: the slot limit n_slots * T then falls between a partial's w
slot and its amp slot in the middle of a voice and of an 8-leaf group, and the reference models it (track_params' limit).
The reference's output must be finite and nonzero in at least half the samples of every voice the hostile values do not touch.

The C++ oracle is sought at single frames of every call -- primed by a one-frame call that requests as many slots as the
engine's limit, so that it drops the same rows; tests/test_track_variants.py pins the reference to it on the CPU.

Ring spans (FR_TRACK_HISTORY, track_variants.SPAN_CASES): voices under a constant Delay, call sequences in which a longer call
grows the delay rings so that the voices' window before idx is rendered from the 64-frame history ring in spans, across its wrap
and from it; every call against the dense reference over absolute frames shifted by the delay AND the oracle over all of it,
with the number and lengths of the bank launches and the tail append asserted."""
import numpy as np
import pytest

import bank_reference
import track_rows
import track_variants
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu

OFFSET = track_rows.OFFSET


class Entry:
    """fill_buffer_dense, the CSR fill_buffer or fill_buffer_device_dense of one renderer."""

    def __init__(self, r, kind):
        self.r, self.kind = r, kind

    def __call__(self, n_slots, idx, m):
        T = m.shape[1]
        if self.kind == "dense":
            return self.r.fill_buffer_dense(n_slots, idx, idx + T, m)
        if self.kind == "csr":
            return self.r.fill_buffer(n_slots, idx, idx + T, list(m))
        assert self.kind == "device_dense", self.kind
        import torch
        d_m = torch.from_numpy(np.ascontiguousarray(m)).cuda()
        d_out = torch.full((n_slots, T), 7.0, dtype=torch.float32, device="cuda")
        s = torch.cuda.current_stream()
        self.r.fill_buffer_device_dense(d_out.data_ptr(), n_slots, T, idx, d_m.data_ptr(), m.shape[0], s.cuda_stream)
        s.synchronize()
        return d_out.cpu().numpy()


def workgroups(b):
    """The workgroups of a reported generated-kernel launch (jit.cpp launch_jit_bank)."""
    tiles = -(-b["frames"] // 64)
    if b["voices_per_wave"]:
        return tiles * -(-b["voices"] // (4 * b["voices_per_wave"]))
    return (tiles * b["voices"]) << b["pieces_log2"]


def seek_frames(m):
    """The first and last frame, the edge of the first tile, and the first frame whose time is not finite."""
    T = m.shape[1]
    odd = np.flatnonzero(~np.isfinite(m[0]))
    return sorted({0, 63, 64, T // 2, T - 1} | set(odd[:1].tolist()))


def check_call(case, hip, entry, ref, limit, idx, m, what, n_slots=None, hostile=()):
    V, P, T = case["V"], case["P"], m.shape[1]
    n_slots = V if n_slots is None else n_slots
    lim = limit.call(n_slots, T)
    got = entry(n_slots, idx, m)
    plan = hip.plan()
    launches = plan["bank_launches"]
    assert len(launches) == 1, f"{what}: ran {launches}"
    b = launches[0]
    assert b["variant"] == case["key"] and b["pieces_log2"] == case["pieces_log2"], f"{what}: ran {b}, expected {case['key']}"
    assert b["kernel"] == "jit_bank" and b["voices"] == V and b["partials"] == P and b["frames"] == T, (what, b)
    assert len(plan["banks"]) == 1 and plan["banks"][0]["tracks"] is True and plan["banks"][0]["jit"], (what, plan["banks"])
    assert plan["pull_rows"] == 0 and plan["track_tail_launches"] == 0, what
    if what == "ramp":   # (the XCD block remap is taken exactly when the count is a multiple of 8)
        assert (workgroups(b) % 8 == 0) == case["xcd"], (what, workgroups(b), b)
    exp = track_rows.expected(V, P, m, lim)
    quiet = track_rows.quiet_voices_sound(exp if lim >= m.shape[0] else exp[:1], hostile)
    assert quiet == "", f"{what}: the reference is silent or not finite where no hostile value is: {quiet}"
    print(f"{case['name']}: {what}: {b['variant']} pieces_log2 {b['pieces_log2']}, {workgroups(b)} workgroups, {T} frames, limit {lim}")
    msg = bank_reference.first_diff(got[:V], exp, f"{case['name']} ({case['key']}) {what} (call at {idx}, {T} frames, limit {lim})")
    assert not msg, msg
    assert not got[V:].any(), f"{what}: output slots beyond the voices are not +0"
    for c in seek_frames(m):
        o = ref.fill_buffer_dense(V, idx + c, idx + c + 1, m[:, c:c + 1])
        msg = bank_reference.first_diff(exp[:, c:c + 1], o, f"{case['name']} {what}: dense reference vs oracle at frame {c}")
        assert not msg, msg
    return exp


def run_case(case, hip_lib, oracle_lib, primed):
    V, P, T, T2 = case["V"], case["P"], case["T"], case["T2"]
    tree = synth.track_tree(V, P)
    seed = P * 7 + V
    with Renderer(hip_lib, options=case["options"]) as hip, Renderer(oracle_lib) as ref:
        hip.set_track_inputs(tree["first_track"])
        synth.install(hip, tree)
        synth.install(ref, tree)
        entry = Entry(hip, case["entry"])
        limit = track_rows.SlotLimit()
        # the oracle drops what the engine drops: one frame, as many slots as the engine's limit will be
        n_prime = track_rows.priming_slots(V, P, T) if primed else V
        ref.fill_buffer_dense(n_prime * T, 0, 1, np.zeros((tree["n_inputs"], 1), np.float32))
        idx = OFFSET
        if primed:
            check_call(case, hip, entry, ref, limit, idx - T, track_rows.regular_rows(V, P, idx - T, T, seed + 1), "priming", n_slots=n_prime)
            assert limit.n_vecs >= tree["n_inputs"]
        check_call(case, hip, entry, ref, limit, idx, track_rows.regular_rows(V, P, idx, T, seed), "ramp")
        m, hostile = track_rows.hostile_rows(case, idx + T, seed)
        check_call(case, hip, entry, ref, limit, idx + T, m, "hostile call", hostile=hostile)
        exp = check_call(case, hip, entry, ref, limit, idx + 2 * T, track_rows.regular_rows(V, P, idx + 2 * T, T2, seed + 2), "second length")
        if not primed:   # the limit matters: the partials beyond it are silent, the last voice altogether
            assert limit.n_vecs == V * T < tree["n_inputs"]
            full = track_rows.expected(V, P, track_rows.regular_rows(V, P, idx + 2 * T, T2, seed + 2))
            assert bank_reference.first_diff(exp, full) and not exp[V - 1].any() and full[V - 1].any()


@pytest.mark.parametrize("case", track_variants.CASES, ids=[c["name"] for c in track_variants.CASES])
def test_track_matrix(hip_lib, oracle_lib, case):
    run_case(case, hip_lib, oracle_lib, primed=True)
    if case["fresh"]:
        run_case(case, hip_lib, oracle_lib, primed=False)


@pytest.mark.parametrize("k", range(len(track_variants.SPAN_CASES)), ids=[c["name"] for c in track_variants.SPAN_CASES])
def test_track_matrix_ring_spans(hip_lib, oracle_lib, k):
    case = track_variants.SPAN_CASES[k]
    V, P, d = track_variants.SPAN_V, track_variants.SPAN_P, case["d"]
    tree = track_rows.span_tree(V, P, d)
    dense = track_rows.SpanReference(V, P, d)
    with Renderer(hip_lib, options={"FR_TRACK_HISTORY": str(case["H"])}) as hip, Renderer(oracle_lib) as ref:
        hip.set_track_inputs(1)
        synth.install(hip, tree)
        synth.install(ref, tree)
        entry = Entry(hip, "device_dense" if k % 2 else "dense")
        head = cap = 0
        for j, (idx, n, n_launches) in enumerate(case["calls"]):
            what = f"{case['name']}: call {j} at {idx}, {n} frames"
            m = track_rows.span_rows(V, P, idx, n, 7 + j)
            got = entry(V, idx, m)
            plan = hip.plan()
            frames, cap = track_rows.span_launches(idx, n, d, head, cap)
            head = idx + n
            launches = plan["bank_launches"]
            assert [b["frames"] for b in launches] == frames and len(frames) == n_launches, (what, launches)
            assert all(b["variant"] == "jit_bank" and b["pieces_log2"] == 0 and b["voices"] == V for b in launches), (what, launches)
            assert len(plan["banks"]) == 1 and plan["banks"][0]["tracks"] is True and plan["banks"][0]["to_ring"], (what, plan["banks"])
            assert plan["pull_rows"] == 0 and plan["track_tail_launches"] == 1 and plan["track_history"] == case["H"], what
            assert plan["track_lookback"] == d and plan["track_tail_bytes"] == 2 * V * P * 64 * 4, what
            print(f"{what}: bank launches of {frames} frames")
            exp = dense.call(idx, m)
            assert track_rows.quiet_voices_sound(exp[:, d:]) == "", what
            msg = bank_reference.first_diff(got, exp, what + ", dense reference")
            assert not msg, msg
            msg = bank_reference.first_diff(got, ref.fill_buffer_dense(V, idx, idx + n, m), what + ", oracle")
            assert not msg, msg
