"""FR_LOOP_DYN on the MI355X: stage_sweep_kernel (option 1) and the windows form on stage_kernel (option 2).

Every case of tests/loop_dyn_cases.py under option 1, on every sample of every call -- first call, ragged steady call, one
frame, a seek past FB_CHUNK, a seek back, a 40 000-frame call that makes the rings grow and wrap, a call with hostile rows --
bit for bit (NaN equals NaN, +0 differs from -0) against
  * the dense forward f32 reference (tests/loop_dyn_reference.py), computed once per case and pinned to the C++ oracle on every
    one of the first frames of the first call;
  * option 2, the independent evaluator that rests on the kernel the other launch forms have proven.
The variant is asserted on the steady launch and on the replay's.  The bank case (synth.feedback_flanger: the bank fills its
ring, then the sweep runs) goes through the same calls in both semantics: on every sample against the windows form and against
the oracle's voices run through the dense forward loops (tests/loop_dyn_cases.py bank_reference), on the first 600 frames
against the oracle's rendering of the whole tree; it shows its bank launch."""
import numpy as np
import pytest

import loop_dyn_cases as L
import loop_dyn_reference as ldr
import stage_reference as sr
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu

_REF = {}


def reference_for(case, oracle_lib):
    if case["key"] not in _REF:
        g = L.build(case)
        rng = np.random.default_rng(11)
        store = sr.InputStore()
        ref = ldr.DenseForward(g, case["semantics"])
        calls = []
        for what, idx, n in L.CALLS:
            rows = L.rows_for(case, what, idx, n, rng)
            store.call(idx, rows)
            exp = ref(store, idx, idx + n)
            exp.setflags(write=False)
            calls.append((what, idx, n, rows, exp))
        m = case["oracle"]                       # pinned once: every one of the first call's first frames
        with Renderer(oracle_lib, semantics=case["semantics"]) as o:
            g.install(o)
            got = o.fill_buffer(g.n_out, 0, m, [r[:m] for r in calls[0][3]])
        msg = sr.first_diff(calls[0][4][:, :m], got, f"{case['key']}: dense forward reference vs the oracle on frames 0..{m - 1}")
        assert not msg, msg
        _REF[case["key"]] = (g, calls, got)
    return _REF[case["key"]]


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_sweep_kernel_against_reference_windows_and_oracle(hip_lib, oracle_lib, case):
    g, calls, oracle = reference_for(case, oracle_lib)
    with Renderer(hip_lib, options=L.SWEEP, semantics=case["semantics"]) as sweep, \
            Renderer(hip_lib, options=L.WINDOWS, semantics=case["semantics"]) as windows:
        g.install(sweep)
        g.install(windows)
        for what, idx, n, rows, exp in calls:
            got = sweep.fill_buffer(g.n_out, idx, idx + n, rows)
            base = windows.fill_buffer(g.n_out, idx, idx + n, rows)
            plan = sweep.plan()
            L.check_plan(case, plan, 1)
            L.check_launches(case, plan, 1, what, n)
            L.check_plan(case, windows.plan(), 2)
            L.check_launches(case, windows.plan(), 2, what, n)
            msg = sr.first_diff(got, exp, f"{case['key']} {what} (call at {idx}, {n} frames): sweep kernel vs the dense forward reference")
            assert not msg, msg
            msg = sr.first_diff(got, base, f"{case['key']} {what} (call at {idx}, {n} frames): sweep kernel vs the windows form")
            assert not msg, msg
            if what == "first":
                m = case["oracle"]
                msg = sr.first_diff(got[:, :m], oracle, f"{case['key']}: sweep kernel vs the oracle on frames 0..{m - 1}")
                assert not msg, msg


@pytest.mark.parametrize("semantics", ["reference", "sparkle"])
def test_bank_voices_through_flangers(hip_lib, oracle_lib, semantics):
    """The bank case through every call of L.CALLS -- the 40 000-frame call grows and wraps rings a bank writes into, the last call's
    time row is hostile --: the sweep kernel on every sample against the composed reference (the oracle's voices through the dense
    forward loops; L.bank_reference pins it to the oracle's rendering of the whole tree on the first 600 frames), against the
    windows form, and against those 600 oracle frames."""
    tree, calls, oracle = L.bank_reference(oracle_lib, semantics)
    V = L.BANK["V"]
    with Renderer(hip_lib, options=L.SWEEP, semantics=semantics) as sweep, Renderer(hip_lib, options=L.WINDOWS, semantics=semantics) as windows:
        synth.install(sweep, tree)
        synth.install(windows, tree)
        for what, idx, n, rows, exp in calls:
            got = sweep.fill_buffer(V, idx, idx + n, rows)
            base = windows.fill_buffer(V, idx, idx + n, rows)
            plan = sweep.plan()
            assert plan["bank_launches"] and plan["banks"][0]["to_ring"] and plan["feedback_loops"] == V, plan
            L.check_plan(L.BANK, plan, 1)
            L.check_launches(L.BANK, plan, 1, what, n)
            L.check_plan(L.BANK, windows.plan(), 2)
            L.check_launches(L.BANK, windows.plan(), 2, what, n)
            msg = sr.first_diff(got, base, f"{L.BANK['key']} [{semantics}] {what}: sweep kernel vs the windows form")
            assert not msg, msg
            msg = sr.first_diff(got, exp, f"{L.BANK['key']} [{semantics}] {what}: sweep kernel vs the oracle's voices through the dense forward loops")
            assert not msg, msg
            if what == "first":
                msg = sr.first_diff(got[:, :len(oracle[0])], oracle, f"{L.BANK['key']} [{semantics}]: sweep kernel vs the oracle on the first frames")
                assert not msg, msg
