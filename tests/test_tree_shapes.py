"""The shape matrix of tests/tree_shapes.py on the CPU: its dense reference (render_shapes, every add the tree's own) against
three other answers bit for bit -- NaN equal to NaN, +0 unequal to -0 -- on a ramp, a hostile row and a row with a run of t = +0.0:
  * the simulator's fr_fill_buffer on every frame: the matcher's real schedule through tests/cpp/sim/sim_kernels.cpp launch_gbank;
  * the C++ oracle, on every frame for the shapes of at most 300 leaves and at seek frames for the larger ones;
  * tests/stage_reference.py's render of the same graph, node by node, for the shapes of at most 300 leaves.
Then what the table claims, asserted from schedule_of (written without csrc/match.cpp): every item size first, in the middle and
last; stack depths 15, 16 and 17; a merge count of 15; runs of big items with and without small ones between; and what
tests/test_hip_tree_shapes.py relies on: the serving prediction against fr_plan_json, that the sum_tree association of the same
leaves is a different answer (sensitivity), that the zero results of the negative-amplitude voices have both signs, and that the
hostile row leaves every voice mostly finite."""
import numpy as np
import pytest

import bank_reference
import sim_tools
import stage_reference
import stream_general_cases as G
import stream_reference
import tree_shapes as TS
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

T, T2 = 130, 70                                          # two tiles and two frames; one tile and six frames
SMALL = 300
SEEKS = (0, 3, 5, 10, 17, 40, 63, 64, 69, 70, 80, 117, 121, 124, 128, T - 1)   # tile boundaries, zero frames, both hostile waves
ROWS = ("ramp", "hostile", "second")


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_BANK_MULTI", "FR_BANK_SHORT", "FR_BANK_TEMPLATE", "FR_STREAM_PROGRAMS", "FR_STREAM_GENERAL", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)


class World:
    """The whole table in one graph -- every shape regular and silent, the variant shapes in every variant -- its rows and
    its reference, made once."""

    def __init__(self):
        self.entries = TS.table_entries(TS.names())
        self.shapes, self.w, self.amp = TS.voices(self.entries)
        self.tree = TS.build_graph(self.shapes, self.w, self.amp)
        self.idx = {"ramp": TS.OFFSET, "hostile": TS.OFFSET + T, "second": TS.OFFSET + 2 * T}
        self.rows = {"ramp": synth.time_ramp(TS.OFFSET, TS.OFFSET + T), "hostile": TS.hostile_row(self.idx["hostile"], T),
                     "second": TS.second_row(self.idx["second"], T2)}
        self.exp = {k: TS.render_shapes(self.shapes, self.w, self.amp, r) for k, r in self.rows.items()}
        # the small shapes: regular and in their variants (a silent copy of every one of them adds nothing node by node)
        self.small = [v for v, s in enumerate(self.shapes) if TS.n_leaves(s) <= SMALL
                      and (self.entries[v][1] != "silent_neg" or self.entries[v][0] in TS.VARIANT_SHAPES)]

    def sub(self, vs):
        """(tree, shapes, w, amp) of the voices vs alone."""
        e = [self.entries[v] for v in vs]
        shapes, w, amp = TS.voices(e, seeds=list(vs))
        return TS.build_graph(shapes, w, amp), shapes, w, amp


@pytest.fixture(scope="module")
def world():
    return World()


def test_hostile_row_is_what_it_says():
    row = TS.hostile_row(TS.OFFSET, T)
    assert all(np.float32(x).tobytes() in {np.float32(y).tobytes() for y in row} for x in np.concatenate([TS.HOSTILE_NEG, TS.HOSTILE_ODD]))
    zeros = [i for i in range(64) if row[i].tobytes() == np.float32(0.0).tobytes()]
    assert zeros == list(TS.ZERO_FRAMES) and len(zeros) <= 4
    row70 = TS.hostile_row(TS.OFFSET, 70)
    assert np.isnan(row70).any() and (row70 < 0).sum() >= len(TS.HOSTILE_NEG)


@pytest.mark.parametrize("what", ROWS)
def test_reference_equals_the_simulator_on_every_frame(sim, world, what):
    V = len(world.shapes)
    with Renderer(sim) as r:
        synth.install(r, world.tree)
        got = r.fill_buffer(V, world.idx[what], world.idx[what] + len(world.rows[what]), [world.rows[what]])
        plan = r.plan()
    msg = bank_reference.first_diff(got, world.exp[what], f"simulator, {what}")
    assert not msg, msg + f" ({world.entries[int(msg.split('voice ')[1].split(',')[0])]})"
    assert plan["pull_rows"] == 0
    # one launch of every voice that goes to its row, one of the voices under depth_17's programs (they go to rings)
    to_ring = sum(len(TS.serving_of(s)[0]) for s in world.shapes if not TS.served(s))
    assert sorted((b["general_tree"], b["to_ring"], b["voices"]) for b in plan["banks"]) == [
        (True, False, sum(TS.served(s) for s in world.shapes)), (True, True, to_ring)], plan["banks"]


@pytest.mark.parametrize("what", ROWS)
def test_reference_equals_the_oracle(oracle_lib, world, what):
    V = len(world.shapes)
    row, idx, exp = world.rows[what], world.idx[what], world.exp[what]
    tree, shapes, w, amp = world.sub(world.small)
    with Renderer(oracle_lib) as o:                       # every frame of the small shapes
        synth.install(o, tree)
        got = o.fill_buffer(len(shapes), idx, idx + len(row), [row])
    msg = bank_reference.first_diff(exp[world.small], got, f"oracle, small shapes, {what}")
    assert not msg, msg
    with Renderer(oracle_lib) as o:                       # the whole table at the seek frames
        synth.install(o, world.tree)
        for c in [c for c in SEEKS if c < len(row)]:
            got = o.fill_buffer(V, idx + c, idx + c + 1, [row[c:c + 1]])
            msg = bank_reference.first_diff(exp[:, c:c + 1], got, f"oracle, {what}, frame {c}")
            assert not msg, msg


def test_reference_equals_stage_reference(world):
    """A second restatement that knows nothing of shapes: the graph itself, node by node, for the regular and the variant
    voices of the small shapes.  stage_reference.render evaluates from frame 0, so the rows' VALUES are fed from frame 0 on: the
    first 40 of the second row (its run of zeros), then the hostile row."""
    vs = world.small
    tree, shapes, w, amp = world.sub(vs)
    row = np.concatenate([world.rows["second"][:40], world.rows["hostile"]])
    got = stage_reference.render(stream_reference.graph_of(tree), [row], 0, len(row))
    exp = TS.render_shapes(shapes, w, amp, row)
    msg = bank_reference.first_diff(got, exp, "stage_reference.render")
    assert not msg, msg
    msg = bank_reference.first_diff(exp[:, 40:], world.exp["hostile"][vs], "the sub-table's voices are the table's")
    assert not msg, msg


def test_table_coverage():
    sch = {n: TS.schedule_of(s) for n, s in TS.TABLE if TS.served(s)}
    first, middle, last = set(), set(), set()
    for s in sch.values():
        if len(s["items"]) >= 3:
            first.add(s["items"][0])
            last.add(s["items"][-1])
            middle.update(s["items"][1:-1])
    every = set(range(TS.MAX_ITEM_LOG2 + 1))
    assert first >= every and middle >= every and last >= every, (first, middle, last)
    depths = {TS.schedule_of(s)["depth"] for _, s in TS.TABLE}
    assert {15, 16, 17} <= depths, depths
    assert max(s["depth"] for s in sch.values()) == 16
    assert TS.is_sum_tree(TS.sum_tree_shape(100)) and TS.is_sum_tree((6, (5, 2))) and not TS.is_sum_tree((6, (2, 5)))
    assert not TS.served(TS.SHAPES["depth_17"]) and TS.served(TS.SHAPES["depth_16"]) and TS.served(TS.SHAPES["depth_15"])
    assert any(15 in s["merges"] for s in sch.values())
    assert any(m == 15 and k >= 5 for s in sch.values() for k, m in zip(s["items"], s["merges"]))      # ... after a split item too

    def longest_big_run(items, allow_small):
        """Most items of >= 32 leaves in a row; with allow_small, small items may stand between them (and at least one does)."""
        best = run = smalls = 0
        for k in items:
            if k >= 5:
                run += 1
                if not allow_small or smalls:
                    best = max(best, run)
            elif allow_small and run:
                smalls += 1
            else:
                run = smalls = 0
        return best
    assert max(longest_big_run(s["items"], False) for s in sch.values()) >= 3
    assert max(longest_big_run(s["items"], True) for s in sch.values()) >= 4
    assert TS.schedule_of(TS.SHAPES["big_run_smalls_between"])["items"] == [5, 0, 6, 2, 5, 4, 7]
    # 2^12 complete leaves are two items of 2048 and a merge
    assert TS.schedule_of(TS.SHAPES["two_2048_and_a_leaf"]) == {"items": [11, 11, 0], "merges": [0, 1, 1], "depth": 2, "offsets": [0, 2048, 4096]}
    leaves = {TS.n_leaves(s) for _, s in TS.TABLE}
    assert {15, 16, 17, 18} <= leaves
    randoms = [s for n, s in TS.TABLE if n.startswith("random_")]
    assert len(randoms) == 30 and all(TS.n_leaves(s) <= 300 for s in randoms)
    # every variant stands on a shape that has its item
    for n in TS.VARIANT_SHAPES:
        assert all(TS.has_variant(TS.SHAPES[n], v) for v in TS.VARIANTS), n
    for n, s in TS.TABLE:                                  # what the builder's operand-order note needs
        assert TS.n_leaves(s) == sum(1 << k for k in TS.schedule_of(s)["items"])


@pytest.mark.parametrize("name", [n for n, _ in TS.TABLE])
def test_serving_prediction_against_the_plan(sim, name):
    shape = TS.SHAPES[name]
    voices, programs = TS.serving_of(shape)
    shapes, w, amp = TS.voices([(name, "regular")])
    with Renderer(sim) as r:
        synth.install(r, TS.build_graph(shapes, w, amp))
        r.fill_buffer(1, 0, 8, [synth.time_ramp(0, 8)])
        plan = r.plan()
    banks = plan["banks"]
    assert [(b["general_tree"], b["voices"], b["partials"]) for b in banks] == [(True, 1, n) for n in voices], (name, banks)
    assert plan["pull_rows"] == 0 and plan["stage_programs"] == programs, (name, plan["stage_programs"], programs)
    if name in ("depth_17", "left_15", "right_15"):
        assert programs == 1
    elif TS.served(shape):
        assert programs == 0 and voices == [TS.n_leaves(shape)]


def test_sensitivity_to_the_association(world):
    """For every served shape of more than 2 items the sum_tree association of the same leaves is another answer on at least
    1 in 20 finite samples (a kernel that summed in the wrong order would be seen).  Two named shapes ARE the sum_tree
    association of their leaves (128 + (2 + 1), 2048 + 2048 + 1), so there the yardstick is the reference itself: they are
    told apart by their form, must differ on no sample, and each has its mirror image in the table."""
    shares = {}
    is_sum_tree = {n for n, s in TS.TABLE if TS.is_sum_tree(s) and len(TS.schedule_of(s)["items"]) > 2}
    assert is_sum_tree == {"128_plus_3", "two_2048_and_a_leaf"} and {"3_plus_128", "leaf_and_two_2048"} <= set(TS.SHAPES)
    for v, (name, variant) in enumerate(world.entries):
        s = world.shapes[v]
        if variant != "regular" or not TS.served(s) or len(TS.schedule_of(s)["items"]) <= 2:
            continue
        other = np.concatenate([TS.render_sum_tree([s], [world.w[v]], [world.amp[v]], world.rows[k])[0] for k in ROWS])
        own = np.concatenate([world.exp[k][v] for k in ROWS])
        fin = np.isfinite(own)
        shares[name] = float((own.view(np.uint32) != other.view(np.uint32))[fin].mean())
        print(f"{name}: {shares[name]:.3f} of the finite samples differ from the sum_tree association")
    assert len(shares) >= 70
    assert all(shares[n] == 0.0 for n in is_sum_tree)
    low = {n: s for n, s in shares.items() if s < 0.05 and n not in is_sum_tree}
    assert not low, low


def test_zero_results_have_both_signs(world):
    """On a frame of t = +0.0 every leaf is a zero with its amplitude's sign, so the root is -0 for the all-negative and the
    silent -0 voices and +0 for every other variant -- the voices with ONE positive amplitude among them.  The hostile row has
    three such frames in a tile (the repair of at most 4 zero frames), the second row six (the pass over all 64 frames)."""
    neg0, pos0 = int(np.float32(-0.0).view(np.uint32)), int(np.float32(0.0).view(np.uint32))
    for what, frames in (("hostile", TS.ZERO_FRAMES), ("second", TS.ZERO_RUN)):
        assert all(world.rows[what][f].tobytes() == np.float32(0.0).tobytes() for f in frames)
        bits = world.exp[what].view(np.uint32)[:, list(frames)]
        seen = {}
        for v, (name, variant) in enumerate(world.entries):
            want = neg0 if np.signbit(TS.ZERO_SIGN[variant]) else pos0
            if variant == "silent_neg" and "shares" in name:       # (the shared sub-tree keeps the first voice's amplitudes)
                want = pos0
            assert (bits[v] == want).all(), (what, name, variant, bits[v])
            seen.setdefault(variant, set()).add(want)
        assert set(seen) == set(TS.VARIANTS)
        assert seen["all_neg"] == {neg0} and all(seen[k] == {pos0} for k in ("one_pos_padded", "one_pos_16", "one_pos_big")), seen
    # a silent voice's roots are zeros on every finite frame, of either sign
    hostile = world.exp["hostile"]
    for v, (name, variant) in enumerate(world.entries):
        if variant in TS.SILENT and "shares" not in name:
            fin = np.isfinite(hostile[v])
            assert fin.sum() > 100 and not hostile[v][fin].any(), name


def test_hostile_rows_leave_the_voices_finite(world):
    for T_ in (T, 70, 200, 961):
        row = TS.hostile_row(TS.OFFSET, T_)
        vs = world.small if T_ > 200 else range(len(world.shapes))
        exp = world.exp["hostile"] if T_ == T else TS.render_shapes([world.shapes[v] for v in vs], [world.w[v] for v in vs], [world.amp[v] for v in vs], row)
        share = np.isfinite(exp).mean(axis=1)
        assert share.min() >= 0.80, (T_, float(share.min()), world.entries[int(np.argmin(share))])
        print(f"hostile row of {T_} frames: at least {share.min():.3f} of every voice's samples are finite")


@pytest.mark.parametrize("patch", sorted(TS.STREAM_PATCHES))
def test_stream_patches_are_served_by_the_schedule_kernel(sim, patch):
    """What tests/test_hip_tree_shapes.py streams: at most 32 voices, every one a schedule voice, no program."""
    entries = TS.STREAM_PATCHES[patch]
    assert len(entries) <= 32
    shapes, w, amp = TS.voices(entries)
    with Renderer(sim, options=G.OPTION) as r:
        synth.install(r, TS.build_graph(shapes, w, amp))
        r.fill_buffer(len(shapes), 0, 64, [synth.time_ramp(0, 64)])
        s = r.plan()["stream"]
    assert s["servable"] and s["kernel"] == G.NEW_KERNEL, s
    assert s["general_voices"] == [TS.n_leaves(x) for x in shapes] and s["programs_per_voice"] == [0] * len(shapes), s
