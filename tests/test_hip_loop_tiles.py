"""FR_LOOP_TILES on the MI355X: stage_tile_kernel (FR_STAGE_JIT=0) and the generated jit_stage_tile (FR_STAGE_JIT=force)
against the dense f32 reference (tests/stage_reference.py) on EVERY output sample, bit for bit (NaN == NaN, +0 != -0).

Every case of tests/loop_tile_cases.py takes the call sequence of tests/test_hip_stage_matrix.py: a first call from frame 0;
the steady call of a ragged length; a 1-frame call; a seek forward past FB_CHUNK (the replay from frame 0 crosses a chunk
boundary and ends in a ragged chunk); a seek back; a call longer than the rings were sized for; a call with a hostile input
row.  Tiled cases assert +tile on the steady launch and on the replay's, the others the reason fr_plan_json gives and that no
launch is tiled.  The reference of a case is computed once and shared by both evaluators; it is pinned to the C++ oracle at
the frames where the oracle's recursion is cheap.

A patch with a bank -- 3 voices of 64 partials through the comb of tools/feedback_bench.py, d = 1 and d = 5 -- is rendered
with the option on and off: the same bits, the oracle's at a few early frames, the plan shows the bank launch and +tile."""
import functools

import numpy as np
import pytest

import loop_tile_cases as L
import stage_reference as sr
import stage_variants as sv
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer
from test_hip_stage_matrix import check_oracle, oracle_frames, rows_for

pytestmark = pytest.mark.gpu

JIT = {"interpreter": "0", "compiled": "force"}


@functools.lru_cache(maxsize=None)
def _max_stride(hip_lib):
    return L.max_stride(hip_lib)


_REFERENCE = {}


def reference_for(case, oracle_lib):
    """The case's calls, their input rows and the dense reference's rows, computed once (and pinned to the oracle once)."""
    if case["key"] in _REFERENCE:
        return _REFERENCE[case["key"]]
    g = L.build(case)
    T = case["T"]
    rng = np.random.default_rng(len(case["key"]) * 7 + T)
    store = sr.InputStore()
    ref = sr.DenseReference(g, case["semantics"])
    calls = [("first", 0, T), ("steady", T, T), ("one frame", 2 * T, 1), ("seek forward", case["seek"], 300), ("seek back", 5, T // 2 + 1),
             ("longer than the rings", 5 + T // 2 + 1, 40000)]
    calls.append(("hostile row", calls[-1][1] + calls[-1][2], T))
    plan = {"fused_stride": 0}
    out = []
    for what, idx, n in calls:
        rows = rows_for(case, idx, n, rng, hostile=what == "hostile row")
        store.call(idx, rows)
        exp = ref(store, idx, idx + n).copy()
        check_oracle(case, oracle_lib, g, store, exp, idx, oracle_frames(case, plan, idx, n, True), True)
        out.append((what, idx, n, rows, exp))
    _REFERENCE[case["key"]] = (g, out)
    return _REFERENCE[case["key"]]


@pytest.mark.parametrize("evaluator", sorted(JIT))
@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_loop_tile_case_against_dense_reference(hip_lib, oracle_lib, case, evaluator):
    case = L.resolve(case, _max_stride(hip_lib))
    g, calls = reference_for(case, oracle_lib)
    jit = evaluator == "compiled"
    with Renderer(hip_lib, options={**L.ON, "FR_STAGE_JIT": JIT[evaluator]}, semantics=case["semantics"]) as hip:
        g.install(hip)
        for what, idx, n, rows, exp in calls:
            got = hip.fill_buffer(g.n_out, idx, idx + n, rows)
            plan = hip.plan()
            forms = L.check_launches(case, plan, what)
            for l in plan["stage_launches"]:
                kernel, form = l["variant"].split("/")
                tiled = "tile" in form.split("+")
                if not jit:
                    assert kernel == "stage_kernel" and plan["stage_jit_form"] is None, (what, l)
                else:
                    f = plan["stage_jit_form"]
                    assert f is not None and f["tile"] == plan["loop_tiles"]["frames"], (what, f, plan["loop_tiles"])
                    assert kernel.startswith("jit_stage["), (what, l)
                    assert (kernel == ("jit_stage[tile,P]" if f["maxp"] else "jit_stage[tile]")) == tiled, (what, l, f)
            if what == "seek forward":
                assert "replay" in forms, forms
            msg = sr.first_diff(got, exp, f"{case['key']} [{evaluator}] {what} (call at {idx}, {n} frames)")
            assert not msg, msg


@pytest.mark.parametrize("evaluator", sorted(JIT))
@pytest.mark.parametrize("d", [1, 5])
def test_bank_voices_through_tiled_combs(hip_lib, oracle_lib, d, evaluator):
    V, P, T = 3, 64, 300
    tree = L.comb_tree(V, P, d)
    calls = [(0, T), (T, T), (2 * T, T), (L.FB_CHUNK + 700, T)]       # from 0, steady, steady, a seek (replay over two chunks)
    with Renderer(hip_lib, options={**L.ON, "FR_STAGE_JIT": JIT[evaluator]}) as on, \
            Renderer(hip_lib, options={"FR_STAGE_JIT": JIT[evaluator]}) as off, Renderer(oracle_lib) as ref:
        for r in (on, off, ref):
            synth.install(r, tree)
        for k, (idx, n) in enumerate(calls):
            t = synth.time_ramp(idx, n)
            got = on.fill_buffer(V, idx, idx + n, [t])
            base = off.fill_buffer(V, idx, idx + n, [t])
            plan = on.plan()
            assert plan["feedback"] and plan["fused_stride"] == d and plan["loop_tiles"]["frames"] == d * (256 // d), plan["loop_tiles"]
            assert plan["bank_launches"] and plan["pull_rows"] == 0, plan
            variants = [l["variant"] for l in plan["stage_launches"]]
            assert any(v.endswith("/feedback+carry_only+tile") for v in variants), variants
            if k == 3:
                assert any(v.endswith("/replay+carry_only+tile") for v in variants), variants
            assert all("tile" not in l["variant"] for l in off.plan()["stage_launches"])
            msg = sr.first_diff(got, base, f"comb d={d} [{evaluator}] call at {idx}: option on vs off")
            assert not msg, msg
            if k == 0:                                                # the oracle's recursion is cheap at the first frames only
                m = 24
                exp = ref.fill_buffer(V, 0, m, [t[:m]])
                msg = sr.first_diff(got[:, :m], exp, f"comb d={d} [{evaluator}]: vs the oracle at frames 0..{m - 1}")
                assert not msg, msg
