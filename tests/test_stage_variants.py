"""The stage-program case table (tests/stage_variants.py) and the dense reference (tests/stage_reference.py), on the CPU.

* The table is well formed: one case per key, each key's kernel and form parse, no key matches UNREACHABLE.
* On the host-logic simulator (engine.cpp's own launch rule, the plain-loop stage_kernel), every case's steady call runs
  its key's launch form and flags, a seek of a feedback case replays with them, and no call of any case runs a launch that
  matches UNREACHABLE.  The simulator has no hipRTC: the jit_stage[...] part of a key is asserted on the GPU.
* The dense reference equals the C++ oracle and oracle/ref_numpy.py bit for bit (NaN == NaN) on every case graph, in short
  call sequences where their recursion is cheap, in both semantics, with hostile input rows and hostile Delay amounts."""
import numpy as np
import pytest

import stage_reference as sr
import stage_variants as sv
from libfriendship_amd.capi import Renderer

KEYS = [c["key"] for c in sv.CASES]


def test_table_is_well_formed():
    assert len(KEYS) == len(set(KEYS)), [k for k in KEYS if KEYS.count(k) > 1]
    forms = {"levels", "fused", "strided", "feedback", "copy", "replay"}
    for c in sv.CASES:
        for key in filter(None, (c["key"], c["replay"])):
            kernel, form = sv.key_base(key).split("/")
            assert kernel == "stage_kernel" or (kernel.startswith("jit_stage[") and kernel.endswith("]")), key
            assert form.split("+")[0] in forms, key
            fb = form.split("+")[0] in ("feedback", "copy", "replay")
            assert sv.unreachable(sv.key_base(key), fb, int(c["options"].get("FR_STAGE_BLOCK", 0))) is None, key
            assert (c["options"].get("FR_STAGE_JIT") == "0") == (kernel == "stage_kernel"), key
        assert c["hoisted"] is None or c["key"].startswith("stage_kernel/"), c
        assert c["graph"][0] in sv.GRAPHS and c["T"] > 0 and c["entry"] in ("host", "dense"), c
        if c["seek"] is not None:
            assert c["seek"] > sv.FB_CHUNK, c
    for pattern, reason in sv.UNREACHABLE.items():
        assert reason, pattern


@pytest.fixture(scope="module")
def sim():
    import sim_tools
    return sim_tools.sim_lib()


def form_of(variant):
    return variant.split("/", 1)[1]


@pytest.mark.parametrize("case", [c for c in sv.CASES if c["graph"][0] != "wide"], ids=[c["key"] for c in sv.CASES if c["graph"][0] != "wide"])
def test_case_reaches_its_form_on_the_simulator(sim, case):
    g = sv.build(case)
    T = case["T"]
    rng = np.random.default_rng(3)
    block = int(case["options"].get("FR_STAGE_BLOCK", 0))
    with Renderer(sim, options=case["options"], semantics=case["semantics"]) as r:
        g.install(r)
        calls = [(0, T), (T, T), (2 * T, 1)]
        if case["seek"] is not None:
            calls.append((case["seek"], 64))
        for n, (idx, n_t) in enumerate(calls):
            rows = [rng.normal(size=n_t).astype(np.float32) for _ in range(case["n_in"])]
            r.fill_buffer(g.n_out, idx, idx + n_t, rows)
            p = r.plan()
            assert p["pull_rows"] == 0, p
            variants = [l["variant"] for l in p["stage_launches"]]
            assert variants, (idx, p)
            for v in variants:
                assert v.startswith("stage_kernel/"), v        # (no hipRTC in the simulator)
                assert sv.unreachable(v, p["feedback"], block, p["fused_carry_only"]) is None, (case["key"], v)
            if case["hoisted"] is not None:
                assert p["stage_hoisted_max"] == case["hoisted"], (case["key"], p["stage_hoisted_max"])
            if n == 1:
                assert form_of(sv.key_base(case["key"])) in map(form_of, variants), (case["key"], variants)
            if n == 3 and case["replay"]:
                assert form_of(case["replay"]) in map(form_of, variants), (case["key"], variants)


def test_grid_split_case_on_the_simulator(sim):
    """66 000 programs in one level: two launches of at most 65535 (grid.y), reported as one with grid_parts 2."""
    case = next(c for c in sv.CASES if c["key"] == "stage_kernel/levels+grid2")
    g = sv.build(case)
    with Renderer(sim, options=case["options"]) as r:
        g.install(r)
        x = np.arange(8, dtype=np.float32)
        got = r.fill_buffer_dense(g.n_out, 0, 8, x.reshape(1, 8))
        p = r.plan()
        assert [l["variant"] for l in p["stage_launches"]] == ["stage_kernel/levels+grid2"], p["stage_launches"]
        assert p["stage_launches"][0]["programs"] == 66000 and p["stage_launches"][0]["grid_parts"] == 2
        exp = sr.render(g, [x], 0, 8)
        msg = sr.first_diff(got, exp, "66000 rows")
        assert not msg, msg


# ---- the reference, pinned to both oracles ------------------------------------------------------------------------
def pin_calls(case):
    """Short calls (the oracles' recursion is cheap): a first call, a contiguous one, a seek forward, a seek back, 1 frame.
    Loops and long delays get lengths past their delays where the recursion stays linear."""
    name, args = case["graph"]
    if name == "echo" and len(args[0]) > 1:
        return [(0, 14), (14, 9), (28, 8), (5, 1)]           # (two taps: the recursion branches)
    if name == "echo":                                       # (one tap: past two trips round the loop)
        n = max(40, 2 * args[0][0] + 9)
        return [(0, n), (n, 23), (2 * n + 300, 17), (9, 1)]
    if name == "wide":
        return [(0, 8), (8, 3), (40, 3)]
    if name in ("rows_inside", "many_inputs") or (name == "many_loads" and len(args) > 1):
        return [(0, 40), (40, 23), (300, 17), (9, 1)]
    if name == "ring_loop":
        return [(0, 45), (45, 20), (200, 9), (3, 1)]
    if name == "chain":
        d = max(args[0])
        return [(0, d + 9), (d + 9, 5), (2 * d + 40, 7), (d - 2, 1)]
    return [(0, 47), (47, 30), (500, 33), (7, 1)]


def hostile_rows(case, n, rng, idx):
    rows = [rng.normal(size=n).astype(np.float32) * 4 for _ in range(case["n_in"])]
    if case["graph"][0] == "dyn_delays":
        for s, amounts in ((1, sv.HOSTILE_AMOUNTS), (2, sv.BOUNDED_AMOUNTS)):
            rows[s] = np.resize(amounts, n).astype(np.float32)
            rows[s][::5] = (np.arange(len(rows[s][::5])) % 9).astype(np.float32)      # (ordinary amounts among them)
        rows[0] = (np.arange(idx, idx + n) % 17).astype(np.float32) - 8
        rows[0][::7] = np.resize(sv.HOSTILE, len(rows[0][::7]))
    else:
        rows[case["hostile"]][:len(sv.HOSTILE)] = sv.HOSTILE[:n]
    return rows


PIN = list({repr(c["graph"]): c for c in sv.CASES}.values())   # every case graph, once


@pytest.mark.parametrize("semantics", ["reference", "sparkle"])
@pytest.mark.parametrize("case", PIN, ids=[f"{c['graph'][0]}{c['graph'][1]}" for c in PIN])
def test_dense_reference_matches_both_oracles(oracle_lib, case, semantics):
    from oracle.ref_numpy import NumpyRefRenderer
    g = sv.build(case)
    rng = np.random.default_rng(11)
    store = sr.InputStore()
    with Renderer(oracle_lib, semantics=semantics) as ref:
        npref = NumpyRefRenderer(semantics)
        g.install(ref)
        g.install(npref)
        for k, (idx, n) in enumerate(pin_calls(case)):
            rows = hostile_rows(case, n, rng, idx) if k != 1 else [rng.normal(size=n).astype(np.float32) for _ in range(case["n_in"])]
            store.call(idx, rows)
            exp = sr.render(g, store.rows, idx, idx + n, semantics)
            o = ref.fill_buffer(g.n_out, idx, idx + n, rows)
            msg = sr.first_diff(exp, o, f"{case['key']} ({semantics}): reference vs C++ oracle, call at {idx} (+{n})")
            assert not msg, msg
            o2 = npref.fill_buffer(g.n_out, idx, idx + n, rows)
            msg = sr.first_diff(exp, o2, f"{case['key']} ({semantics}): reference vs ref_numpy, call at {idx} (+{n})")
            assert not msg, msg


def test_dense_reference_long_loop_is_fast():
    """A 40 000-frame two-tap loop takes well under the recursion's exponential time, and equals a scalar f32 loop over every
    frame (the oracles pin the same graph on short calls above)."""
    import time
    g = sv.GRAPHS["echo"]((3, 6))
    x = np.random.default_rng(2).normal(size=40000).astype(np.float32)
    t0 = time.perf_counter()
    out = sr.render(g, [x], 0, 40000)
    assert time.perf_counter() - t0 < 5.0
    y = np.zeros(40000, np.float32)
    for t in range(40000):     # x = in0 + (0.5 * D(x, 3) + 0.25 * D(x, 6)), in the graph's order
        a = np.float32(0.5) * (y[t - 3] if t >= 3 else np.float32(0))
        b = np.float32(0.25) * (y[t - 6] if t >= 6 else np.float32(0))
        y[t] = x[t] + (a + b)
    msg = sr.first_diff(out, y.reshape(1, -1), "two-tap loop vs scalar loop")
    assert not msg, msg
