"""The planner's proofs on an MI355X (tables: tests/proof_cases.py; the CPU legs and the shared drivers: tests/test_proofs_sim.py).

  B  every row of MOD1_DIVIDENDS as a generated voice kernel against the oracle, in range (where a FAST row's waves take the
     v_fract_f32 body) and hostile; fast_ok and jit asserted from fr_plan_json.  One lane out of range: a single value outside
     [+0, 2^32] in one lane of an in-range call must send that wave to the general body -- a per-wave vote that looked at one
     lane, or a FRACT_INPUTS mask that missed an input, gives +0 for -0 (and worse) exactly there.  The same through
     jit_bank_multi, through a voice's ring and through the hand-written bank_kernel.
  C  BOUNDED_AMOUNTS, the loop that reaches its lower bound, and a streamed Delay(In0, Modulo(In1, 48)).
  D  observed hulls through input_range_kernel: an extreme in one element at lane, wave, block and grid-stride edges, the flags,
     more than RANGE_MAX_ROWS rows, the rebuild from stored history."""
import numpy as np
import pytest

import proof_cases as pc
import test_proofs_sim as S
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu
pp = pc.pp


# ---- B: the sign rule --------------------------------------------------------------------------------------------------------------
MOD1_GROUPS = [(cls, i, chunk) for cls in ("FAST", "NOT", "FREE") for i, chunk in enumerate(pc.chunks(pc.mod1_items(cls)))]


@pytest.mark.parametrize("cls,part,items", MOD1_GROUPS, ids=[f"{cls}{i}" for cls, i, _ in MOD1_GROUPS])
def test_modulo_by_one_dividends(hip_lib, oracle_lib, cls, part, items):
    calls = (("in range", list(pc.in_range_rows())), ("hostile", list(pc.hostile_rows())))
    for row, semantics in items:
        tree = pc.voice_tree(pc.leaf_of(row["D"]))
        with Renderer(hip_lib, options=row["options"], semantics=semantics) as r, Renderer(oracle_lib, semantics=semantics) as o:
            synth.install(r, tree)
            synth.install(o, tree)
            for what, rows in calls:
                got = r.fill_buffer(1, 0, len(rows[0]), rows)
                exp = o.fill_buffer(1, 0, len(rows[0]), rows)
                msg = pp.first_diff("Modulo(D, 1)", f"D = {row['name']} ({semantics}, {what})", rows[0], rows[1], got[0], exp[0])
                assert not msg, msg
            plan = r.plan()
        banks = plan["banks"]
        assert plan["pull_rows"] == 0 and not plan["stage_launches"] and len(banks) == 1, (row["name"], plan["pull_rows"], banks)
        assert banks[0]["jit"] and banks[0]["partials"] == pc.P and banks[0]["voices"] == 1, banks
        assert all(l["kernel"] == "jit_bank" for l in plan["bank_launches"]) and plan["bank_launches"], plan["bank_launches"]
        if cls == "FREE":
            print(f"FREE row {row['name']} ({semantics}): fast_ok = {banks[0]['fast_ok']}")
        else:
            assert banks[0]["fast_ok"] == (cls == "FAST"), (row["name"], semantics, banks)


# ---- B: one lane out of range ------------------------------------------------------------------------------------------------------
def planted_calls(r, o, n_rows, n_in, start=0, whole_calls=False):
    """Every planted call on renderer r against the oracle o.  The expectation is the oracle's in-range call with the planted
    frame's column replaced by the oracle's rendering of that one frame (a voice has no memory); whole_calls: the oracle renders
    every call whole (a Delay has)."""
    T = pc.PLANT_T
    base = pc.plant_base_rows(T, start)[:n_in]
    exp_base = o.fill_buffer(n_rows, start, start + T, base)
    got = r.fill_buffer(n_rows, start, start + T, base)
    assert not pp.differing(got, exp_base).any(), "the in-range call"
    n = 0
    for slot, frame, value in pc.plants(n_in):
        rows = [b.copy() for b in base]
        rows[slot][frame] = value
        if whole_calls:
            exp = o.fill_buffer(n_rows, start, start + T, rows)
        else:
            exp = exp_base.copy()
            exp[:, frame] = o.fill_buffer(n_rows, start + frame, start + frame + 1, [x[frame:frame + 1] for x in rows])[:, 0]
        got = r.fill_buffer(n_rows, start, start + T, rows)
        bad = pp.differing(got, exp)
        assert not bad.any(), (f"In{slot}[{frame}] = {value!r}: {int(bad.sum())} samples differ, first at {np.argwhere(bad)[0].tolist()}: "
                               f"got {got[tuple(np.argwhere(bad)[0])]!r}, expected {exp[tuple(np.argwhere(bad)[0])]!r}")
        n += 1
    return n


@pytest.mark.parametrize("name", list(pc.PLANT_VOICES))
def test_one_lane_out_of_range(hip_lib, oracle_lib, name):
    assert S.planted_minus_zero_shows(oracle_lib) == pc.PLANT_FRAMES[0]      # on the CPU first: the planted -0.0 CAN fail
    leaf, n_in, _ = pc.PLANT_VOICES[name]
    tree = pc.voice_tree(leaf)
    with Renderer(hip_lib) as r, Renderer(oracle_lib) as o:
        synth.install(r, tree)
        synth.install(o, tree)
        assert planted_calls(r, o, 1, n_in) == n_in * len(pc.PLANT_FRAMES) * len(pc.PLANT_VALUES)
        plan = r.plan()
    assert len(plan["banks"]) == 1 and plan["banks"][0]["jit"] and plan["banks"][0]["fast_ok"], plan["banks"]
    assert [l["variant"] for l in plan["bank_launches"]] == ["jit_bank"], plan["bank_launches"]


def test_one_lane_out_of_range_whole_voices_per_wave(hip_lib, oracle_lib):
    """jit_bank_multi, at the smallest voice count whose plan reports it (one voice fewer: jit_bank)."""
    assert S.planted_minus_zero_shows(oracle_lib) == pc.PLANT_FRAMES[0]
    V = pc.multi_voices()
    wv = ("col", pc.W_COL)
    leaf = pc.leaf_of(("Multiply", pc.X, wv))
    for n, variant in ((V - 1, "jit_bank"), (V, "jit_bank_multi")):
        tree = pc.voice_tree(leaf, n, cols={id(wv): pc.voice_cols(n)})
        with Renderer(hip_lib) as r, Renderer(oracle_lib) as o:
            synth.install(r, tree)
            synth.install(o, tree)
            if n == V:
                planted_calls(r, o, n, 1)
            else:
                r.fill_buffer(n, 0, pc.PLANT_T, pc.plant_base_rows()[:1])
            plan = r.plan()
        assert sum(b["voices"] for b in plan["banks"]) == n and all(b["jit"] and b["fast_ok"] for b in plan["banks"]), plan["banks"]
        assert [l["variant"] for l in plan["bank_launches"]] == [variant] * len(plan["bank_launches"]) and plan["bank_launches"], (n, plan["bank_launches"])


def test_one_lane_out_of_range_through_a_ring(hip_lib, oracle_lib):
    """The voice feeds a Delay of 100 frames and the call comes right after a seek: the bank writes a ring (to_ring) whose window
    starts 100 frames before the call, so the planted frame sits in another lane of another wave than in the call."""
    assert S.planted_minus_zero_shows(oracle_lib) == pc.PLANT_FRAMES[0]
    tree = pc.delayed_voice_tree(pc.PLANT_VOICES["x*w"][0])
    with Renderer(hip_lib) as r, Renderer(oracle_lib) as o:
        synth.install(r, tree)
        synth.install(o, tree)
        planted_calls(r, o, 1, 1, start=pc.DELAYED_VOICE_START, whole_calls=True)
        plan = r.plan()
    assert len(plan["banks"]) == 1 and plan["banks"][0]["jit"] and plan["banks"][0]["fast_ok"] and plan["banks"][0]["to_ring"], plan["banks"]
    assert plan["max_lookback"] == pc.DELAYED_VOICE_FRAMES and plan["pull_rows"] == 0, plan["max_lookback"]
    assert plan["bank_launches"] and all(l["frames"] > pc.PLANT_T for l in plan["bank_launches"]), plan["bank_launches"]


def test_one_lane_out_of_range_hand_written_bank_kernel(hip_lib, oracle_lib):
    """synth.additive_tree through the template matcher: bank_kernel's own vote (__all over the time row's lanes)."""
    tree = synth.additive_tree(n_voices=2, n_partials=64, seed=1)
    with Renderer(hip_lib) as r, Renderer(oracle_lib) as o:
        synth.install(r, tree)
        synth.install(o, tree)
        planted_calls(r, o, 2, 1)
        plan = r.plan()
    assert len(plan["banks"]) == 1 and not plan["banks"][0]["jit"] and plan["banks"][0]["fast_ok"], plan["banks"]
    assert [l["kernel"] for l in plan["bank_launches"]] == ["bank_kernel"], plan["bank_launches"]


# ---- C: bounds that are attained --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stage_jit", ["0", "force"])
@pytest.mark.parametrize("semantics", pp.SEMANTICS)
@pytest.mark.parametrize("name,A,top", pc.BOUNDED_AMOUNTS, ids=[b[0] for b in pc.BOUNDED_AMOUNTS])
def test_bounded_amounts_reach_their_top(hip_lib, name, A, top, semantics, stage_jit):
    S.run_bounded_amount(hip_lib, name, A, top, semantics, stage_jit, compiled=True)


def test_a_loop_whose_amount_reaches_its_lower_bound(hip_lib):
    S.run_dyn_loop(hip_lib)


def test_streamed_delay_of_the_time_row_reaches_its_bound(hip_lib, oracle_lib):
    """Row v = voice_v + Delay(In0, Modulo(In1, 48)) under block streaming with FR_STREAM_HISTORY: In1 = -1e-45 makes the amount
    exactly 48.0, the stream's input_lookback covers it, and the blocks equal fr_fill_buffer's and the oracle's."""
    import stream_dyn_cases as SD
    import stream_hist_cases as SH
    V, B, n_blocks = 2, pp.STREAM_BLOCK, 6
    g = synth.GraphArrays()
    v = SH._voices(g, V, 128)
    amount = g.binop(synth.K_MOD, synth.IN(1), synth.C(np.array([48.0], np.float32)), 1)
    dl = g.nodes(synth.K_DELAY, 1)
    g.edge(0, dl, 0, 0)
    g.edge(amount, dl, 0, 1)
    tree = SD._to_rows(g, g.binop(synth.K_SUM2, v, np.broadcast_to(dl, (V,)), V))
    N = B * n_blocks
    rows = [synth.time_ramp(0, N), np.resize(np.concatenate([pc.AMOUNT_DRIVERS, np.array([3.0, 47.5, 17.25, np.nan, -2.0, np.inf], np.float32)]), N)]
    frames = pc.frames_of(pp.reference("Modulo", rows[1], np.float32(48.0)))
    assert frames.max() == 48 and (frames[48:] == 48).any()
    with Renderer(hip_lib) as f, Renderer(oracle_lib) as o:
        synth.install(f, tree)
        synth.install(o, tree)
        filled = f.fill_buffer(V, 0, N, rows)
        exp = o.fill_buffer(V, 0, N, rows)
    got, plan = pp.stream_blocks(hip_lib, tree, V, rows, dict(SH.DYN, **SH.IDLE))
    s = plan["stream"]
    assert s["servable"] and s["kernel"] == SH.NEW_KERNEL and s["hist_dyn_reads"] == V and s["input_lookback"] >= 48, s
    assert not pp.differing(got, filled).any() and not pp.differing(got, exp).any(), np.argwhere(pp.differing(got, exp))[:4].tolist()


# ---- D: observed hulls ---------------------------------------------------------------------------------------------------------------
JIT_OFF = {"FR_STAGE_JIT": "0"}      # (the edge cases make a renderer each: the interpreter spares them a run-time compile each)


@pytest.mark.parametrize("L", pc.SPIKE_LENGTHS)
def test_observed_hull_spike_at_every_edge(hip_lib, oracle_lib, L):
    assert S.run_spike_edges(hip_lib, oracle_lib, L, JIT_OFF) == 2 * len(pc.spike_positions(L))


def test_observed_hull_longest_row(hip_lib, oracle_lib):
    """More than 64 blocks' worth: every block strides on past the grid (the tail past 64 * 16384), the compiled stage program on."""
    L = pc.SPIKE_LONGEST
    for k, pos in enumerate(pc.spike_positions(L) + [64 * pc.RANGE_BLOCK - 1, 64 * pc.RANGE_BLOCK]):
        pl = S.spike_case(hip_lib, oracle_lib, L, pos, 5.0, S.ENTRIES[k % 2])
        assert pl["observed_lookback"] == 8 and pl["pull_rows"] == 0 and pl["range_launches"] > 0, (pos, pl["observed_lookback"], pl["pull_rows"])


def test_observed_hull_negative_extreme(hip_lib, oracle_lib):
    S.run_negative_extreme(hip_lib, oracle_lib, JIT_OFF)


def test_observed_hull_flags_at_the_last_element(hip_lib, oracle_lib):
    S.run_flags_at_the_last_element(hip_lib, oracle_lib, JIT_OFF)


def test_observed_hull_33_slots_two_launches(hip_lib, oracle_lib):
    S.run_33_slots(hip_lib, oracle_lib)


def test_observed_hull_rebuilt_from_stored_history(hip_lib, oracle_lib):
    for spike_at in S.REBUILD_SPIKES:
        S.run_rebuild(hip_lib, oracle_lib, spike_at=spike_at)
