"""Every stage-program launch form the rule can pick (tests/stage_variants.py), on the MI355X, against the dense f32
reference (tests/stage_reference.py) on EVERY output sample, bit for bit (NaN == NaN, +0 != -0).

Per case the renderer gets the case's options, and each call asserts from fr_plan_json's "stage_launches" that no launch
matches UNREACHABLE and that every launch ran the case's kernel (jit_stage cases: the generated form its key names, the
same as "stage_jit_form").  Calls: a first call from frame 0 (reads before frame 0 are +0); the steady call of a ragged
length, which runs the case's key; a 1-frame call; a seek forward (feedback cases: past FB_CHUNK, so the replay from frame 0
crosses a chunk boundary, and runs the case's replay key); a seek back; a call longer than the rings were sized for (they
are re-allocated); a call with a hostile input row (NaN, +-inf, +-0, subnormals, 1e30, 3e38; a Delay amount's row: NaN, -0,
negative, fractional, 2^64, +inf).  The C++ oracle is sought at the first and last frame of each call and at the stride
boundaries, given the input history the frame depends on; for feedback cases only at frames where its recursion is cheap.
That pins the reference to the oracle on the GPU's own rows."""
import numpy as np
import pytest

import stage_reference as sr
import stage_variants as sv
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu

FB_ORACLE_FRAMES = 40          # feedback: the oracle's recursion is sought only below this frame
LOOKBACK = {"chain": lambda a: sum(a[0]), "many_loads": lambda a: a[0] + 1, "delayed_reads": lambda a: a[0] + 1, "many_inputs": lambda a: 1,
            "dyn_delays": lambda a: 2 + 64, "wide": lambda a: a[1] if len(a) > 1 else 3}


def rows_for(case, idx, n, rng, hostile=False):
    rows = [(rng.normal(size=n) * 3).astype(np.float32) for _ in range(case["n_in"])]
    if case["graph"][0] == "dyn_delays":   # amounts: whole and fractional frames below 64, some negative
        for s, amounts in ((1, sv.HOSTILE_AMOUNTS), (2, sv.BOUNDED_AMOUNTS)):
            rows[s] = (rng.integers(-8, 60, size=n) + rng.integers(0, 4, size=n) * 0.25).astype(np.float32)
            if hostile:
                rows[s][1::3] = np.resize(amounts, len(rows[s][1::3]))
    if hostile:
        s = 0 if case["graph"][0] == "dyn_delays" else case["hostile"]
        rows[s][::5] = np.resize(sv.HOSTILE, len(rows[s][::5]))
    return rows


def oracle_frames(case, plan, idx, n, feedback):
    stride = plan.get("fused_stride") or 0
    c = {idx, idx + n - 1, idx + n // 2}
    for k in (1, 2, 3):
        if stride:
            c |= {idx + k * stride - 1, idx + k * stride}
        c.add(idx + 64 * k)
    c = {t for t in c if idx <= t < idx + n}
    if feedback:
        c = {t for t in c if t < FB_ORACLE_FRAMES} | {t for t in range(idx, min(idx + n, FB_ORACLE_FRAMES), 7)}
    return sorted(c)


def check_oracle(case, oracle_lib, g, store, exp, idx, frames, feedback):
    """The oracle at absolute frame t, from a fresh renderer given the stored input rows the frame depends on."""
    name, args = case["graph"]
    n_in = case["n_in"]
    for t in frames:
        a = 0 if feedback else max(0, t - max(LOOKBACK[name](args), n_in))
        e = min(max(t + 1, a + n_in), len(store.rows[0]))   # (the store keeps n_slots * n_times rows at most)
        with Renderer(oracle_lib, semantics=case["semantics"]) as o:
            g.install(o)
            got = o.fill_buffer(g.n_out, a, e, [r[a:e] for r in store.rows])
        msg = sr.first_diff(exp[:, t - idx:t - idx + 1], got[:, t - a:t - a + 1],
                            f"{case['key']}: dense reference vs oracle at frame {t}")
        assert not msg, msg


def kernel_of(key):
    return sv.key_base(key).split("/")[0]


@pytest.mark.parametrize("case", sv.CASES, ids=[c["key"] for c in sv.CASES])
def test_stage_variant_against_dense_reference(hip_lib, oracle_lib, case):
    g = sv.build(case)
    T = case["T"]
    rng = np.random.default_rng(len(case["key"]) * 7 + T)
    store = sr.InputStore()
    ref = sr.DenseReference(g, case["semantics"])
    block = int(case["options"].get("FR_STAGE_BLOCK", 0))
    feedback_case = case["seek"] is not None
    seek = case["seek"] if feedback_case else 5000 + T
    wide = case["graph"][0] == "wide"
    calls = [("first", 0, T), ("steady", T, T), ("one frame", 2 * T, 1), ("seek forward", seek, 300),
             ("seek back", 5, T // 2 + 1)]
    if wide:   # (66 000 rows: short calls; they read no ring)
        calls[3] = ("seek forward", 300, 40)
    else:
        calls.append(("longer than the rings", 5 + T // 2 + 1, 40000 if feedback_case else 6000))
    last = calls[-1]
    calls.append(("hostile row", last[1] + last[2], T))
    with Renderer(hip_lib, options=case["options"], semantics=case["semantics"]) as hip:
        g.install(hip)
        for what, idx, n in calls:
            rows = rows_for(case, idx, n, rng, hostile=what == "hostile row")
            store.call(idx, rows)
            if case["entry"] == "dense":
                got = hip.fill_buffer_dense(g.n_out, idx, idx + n, np.stack(rows))
            else:
                got = hip.fill_buffer(g.n_out, idx, idx + n, rows)
            plan = hip.plan()
            launches = plan["stage_launches"]
            variants = [l["variant"] for l in launches]
            assert plan["pull_rows"] == 0 and variants, (what, plan)
            assert plan["feedback"] == feedback_case, (what, plan["feedback"])
            kern = kernel_of(case["key"])
            for v in variants:
                assert sv.unreachable(v, plan["feedback"], block, plan["fused_carry_only"]) is None, (case["key"], what, v)
                assert v.split("/")[0] == kern, f"{what}: ran {variants}, expected kernel {kern}"
            if kern.startswith("jit_stage"):
                f = plan["stage_jit_form"]
                flags = kern[len("jit_stage["):-1].split(",")
                assert flags == (["deep"] if f["deep"] else ["plain"]) + (["P"] if f["maxp"] else []) + (["defer"] if f["defer"] else []) + \
                    [f"B{f['blk']}"], (kern, f)
            else:
                assert plan["stage_jit_form"] is None, plan["stage_jit_form"]
            if case["hoisted"] is not None:
                assert plan["stage_hoisted_max"] == case["hoisted"], (what, plan["stage_hoisted_max"])
            if what == "steady":
                assert sv.key_base(case["key"]) in variants, f"steady call ran {variants}, expected {case['key']}: {launches}"
            if what == "seek forward" and case["replay"]:
                assert case["replay"] in variants, f"seek ran {variants}, expected {case['replay']}"
            if what == "seek forward" and feedback_case:
                assert any(l["form"] == "replay" for l in launches), variants
            exp = ref(store, idx, idx + n)
            msg = sr.first_diff(got, exp, f"{case['key']} {what} (call at {idx}, {n} frames)")
            assert not msg, msg
            if not wide:
                check_oracle(case, oracle_lib, g, store, exp, idx, oracle_frames(case, plan, idx, n, feedback_case), feedback_case)
