"""The planner's proofs on the CPU (tests/proof_cases.py has the tables; tests/test_hip_proofs.py runs them on the MI355X).

  A  tests/cpp/range_tests.cpp: Range::combine sound for one step and for chains, not vacuous, and converted to frames as
     stage.cpp converts it.
  B  the sign rule: BankMatcher's fast_ok for every row of MOD1_DIVIDENDS (through tests/cpp/voice_proof.cpp: the simulator has
     no run-time compiler, so its plans hold no generated voice and its fr_plan_json no fast_ok for one) equals the row's class;
     and, independently of the rule, the oracle's rendering of D itself over inputs in [+0, 2^32] is finite with the sign bit
     clear wherever fast_ok is true, and offends at every NOT row's witness.
  C  BOUNDED_AMOUNTS on the host-logic simulator: the amount attains the top of its interval, the planned look-back covers it,
     every frame equals the dense forward reference; a loop through a Delay whose amount reaches its proven lower bound.
  D  the drivers of the observed-hull cases, run here on the simulator for the host's part of them (which rows are reduced, in how
     many launches, the rebuild from stored history): the simulator reduces a row with a host loop, so input_range_kernel itself
     is tests/test_hip_proofs.py's."""
import json
import os
import subprocess

import numpy as np
import pytest

import loop_dyn_reference as ldr
import proof_cases as pc
import sim_tools
import stage_reference as sr
from libfriendship_amd import synth
from libfriendship_amd.capi import FR_ERR_CYCLE, RenderError, Renderer
from observed_delay_cases import Pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")


def _host_program(name, sources, opt):
    src = os.path.join(ROOT, "tests", "cpp", name + ".cpp")
    out = os.path.join(BUILD, name)
    deps = [src] + [os.path.join(CSRC, f) for f in sources]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run(["g++", "-std=c++17", opt, "-ffp-contract=off", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-Wno-subobject-linkage",
                        "-pthread", "-o", out, src, "-ldl"], check=True)
    return out


HOST_SOURCES = ("graph.cpp", "graph.hpp", "match.cpp", "match.hpp", "stage.cpp", "stage.hpp", "stagejit.cpp", "leafjit.cpp", "range.hpp", "jit.hpp",
                "kernels.hpp")


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


# ---- A ----------------------------------------------------------------------------------------------------------------------------
def test_interval_arithmetic_is_sound_and_not_vacuous():
    p = subprocess.run([_host_program("range_tests", HOST_SOURCES, "-O2")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "3 passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
    line = next(l for l in p.stdout.splitlines() if l.startswith("one step:"))
    ranges, finite, checks = (int(line.split(w)[0].split()[-1].strip("(")) for w in (" ranges", " finite", " checks"))
    assert checks >= 5 * 10 ** 7 and 4 * finite >= ranges, line


# ---- B ----------------------------------------------------------------------------------------------------------------------------
def _graph_text(tree, sparkle, n_slots):
    lines = [f"graph {int(sparkle)} {n_slots}"]
    lines += [f"n {h} {k}" for h, k in zip(tree["handles"].tolist(), tree["kinds"].tolist())]
    lines += ["e %d %d %d %d" % tuple(e) for e in tree["edges"].tolist()]
    return "\n".join(lines + ["end"])


def voice_proofs(leaves_and_semantics):
    """What BankMatcher proves of each (leaf expression, semantics): the dicts tests/cpp/voice_proof.cpp prints."""
    text = "\n".join(_graph_text(pc.voice_tree(leaf), s == "sparkle", 1) for leaf, s in leaves_and_semantics)
    p = subprocess.run([_host_program("voice_proof", HOST_SOURCES, "-O1")], input=text + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = [json.loads(l) for l in p.stdout.splitlines()]
    assert len(out) == len(leaves_and_semantics)
    return out


@pytest.fixture(scope="module")
def mod1_proofs():
    items = [(r, s) for r in pc.MOD1_DIVIDENDS for s in r["semantics"]]
    return {(r["name"], s): p for (r, s), p in zip(items, voice_proofs([(pc.leaf_of(r["D"]), s) for r, s in items]))}


def test_the_table_has_four_free_rows():
    assert [r["cls"] for r in pc.MOD1_DIVIDENDS].count("FREE") == pc.N_FREE == 4
    assert all(r["cls"] in ("FAST", "NOT", "FREE") and (r["witness"] is not None) == (r["cls"] == "NOT") for r in pc.MOD1_DIVIDENDS)
    assert len({r["name"] for r in pc.MOD1_DIVIDENDS}) == len(pc.MOD1_DIVIDENDS)


@pytest.mark.parametrize("row", pc.MOD1_DIVIDENDS, ids=[r["name"] for r in pc.MOD1_DIVIDENDS])
def test_sign_rule_against_the_oracle(oracle_lib, mod1_proofs, row):
    rows = list(pc.in_range_rows())
    tree = pc.dividend_rows_tree(row["D"])
    for semantics in row["semantics"]:
        proof = mod1_proofs[(row["name"], semantics)]
        assert proof["matched"] and proof["jit"] and proof["has_mod1"] and proof["log2_p"] == 5, proof
        if row["cls"] != "FREE":
            assert proof["fast_ok"] == (row["cls"] == "FAST"), (row["name"], semantics, proof)
        else:
            print(f"FREE row {row['name']} ({semantics}): fast_ok = {proof['fast_ok']}")
        with Renderer(oracle_lib, semantics=semantics) as o:
            synth.install(o, tree)
            d = o.fill_buffer(len(pc.WATCHED), 0, len(rows[0]), rows)
            # (the table's own arithmetic: D by the float64 reference is what the oracle renders)
            for i, k in enumerate(pc.WATCHED):
                exp = np.broadcast_to(pc.evaluate(row["D"], rows, k, semantics), d[i].shape)
                assert not pc.pp.differing(d[i], exp).any(), (row["name"], semantics, k)
            # soundness, whatever the rule is: a voice that may take the fract body never hands it an offending dividend
            if proof["fast_ok"]:
                bad = pc.offends(d)
                assert not bad.any(), (row["name"], semantics, [(pc.WATCHED[i], float(rows[0][t]), float(rows[1][t]), float(d[i, t])) for i, t in np.argwhere(bad)[:4]])
            if row["cls"] == "FREE":      # the class's claim: never an offending D on these inputs either
                assert not pc.offends(d).any(), (row["name"], semantics)
            if row["cls"] == "NOT":       # the witness does what the table says it does
                x, y = (np.array([v], np.float32) for v in row["witness"])
                assert x[0].view(np.uint32) <= 0x4F800000 and y[0].view(np.uint32) <= 0x4F800000
                w = o.fill_buffer(len(pc.WATCHED), 0, 1, [x, y])
                assert pc.offends(w).any(), (row["name"], semantics, w.tolist())


def test_sign_rule_is_sound_on_random_dividends(oracle_lib):
    """The soundness statement again, on 300 seeded dividends of depth <= 3 that no table lists: wherever the matcher says fast_ok,
    the oracle's D over the in-range inputs is finite with the sign bit clear.  (Whether the rule COULD have said fast_ok is the
    table's business.)"""
    rng = np.random.default_rng(0x5EED0B04)
    leaves = [pc.X, pc.X, pc.Y, pc.W] + [pc.c(v) for v in (0.25, 0.75, 1.0, 2.0, 5.0, 0.0, -0.0, -0.5, -1.0, 3e38, np.inf, np.nan)]

    def random_d(depth):
        if depth == 0 or (depth < 3 and rng.integers(4) == 0):
            return leaves[rng.integers(len(leaves))]
        return (pc.pp.OPS[rng.integers(len(pc.pp.OPS))], random_d(depth - 1), random_d(depth - 1))

    def reads_input(e):
        return e[0] == "in" or (e[0] in pc.pp.OPS and (reads_input(e[1]) or reads_input(e[2])))

    items = []
    while len(items) < 300:
        D = random_d(3)
        if reads_input(D):
            items += [(D, s) for s in (pc.pp.SEMANTICS if pc.has_op(D, "Minimum") else pc.pp.SEMANTICS[:1])]
    proofs = voice_proofs([(pc.leaf_of(D), s) for D, s in items])
    rows = list(pc.in_range_rows())
    n_fast = n_not = 0
    for (D, semantics), proof in zip(items, proofs):
        if not (proof["matched"] and proof["jit"] and proof["has_mod1"]):
            continue                                  # (leaves the lowering folded or merged: no generated voice, no claim)
        n_fast += proof["fast_ok"]
        n_not += not proof["fast_ok"]
        if proof["fast_ok"]:
            with Renderer(oracle_lib, semantics=semantics) as o:
                synth.install(o, pc.dividend_rows_tree(D))
                d = o.fill_buffer(len(pc.WATCHED), 0, len(rows[0]), rows)
            bad = pc.offends(d)
            assert not bad.any(), (D, semantics, [(float(rows[0][t]), float(rows[1][t]), float(d[i, t])) for i, t in np.argwhere(bad)[:4]])
    assert n_fast >= 1 and n_not >= 1, (n_fast, n_not)
    print(f"{n_fast} random dividends with fast_ok, {n_not} without")


def test_fract_inputs_are_the_inputs_of_the_dividends():
    """FRACT_INPUTS (the inputs the per-wave vote tests) of the three planted voices: exactly the inputs under a Modulo(., 1)."""
    names = list(pc.PLANT_VOICES)
    for name, proof in zip(names, voice_proofs([(pc.PLANT_VOICES[n][0], "reference") for n in names])):
        leaf, n_in, fract = pc.PLANT_VOICES[name]
        assert proof["matched"] and proof["jit"] and proof["fast_ok"] and proof["has_mod1"], (name, proof)
        assert sorted(proof["fract_slots"]) == list(fract) and sorted(proof["input_slots"]) == list(range(n_in)), (name, proof)


def planted_minus_zero_shows(oracle_lib):
    """The planted -0.0 CAN fail: with the fract body (a - floorf(a)) at that frame the voice x*w is +0 where the oracle has -0,
    and nowhere else do the two differ.  Returns the frame."""
    rows = pc.plant_base_rows()
    frame = pc.PLANT_FRAMES[0]
    rows[0][frame] = -0.0
    with Renderer(oracle_lib) as o:
        synth.install(o, pc.voice_tree(pc.PLANT_VOICES["x*w"][0]))
        exp = o.fill_buffer(1, 0, pc.PLANT_T, rows[:1])[0]
    alt = pc.fract_body_voice(rows[0])
    diff = np.flatnonzero(exp.view(np.uint32) != alt.view(np.uint32))
    assert diff.tolist() == [frame] and exp.view(np.uint32)[frame] == 0x80000000 and alt.view(np.uint32)[frame] == 0, (diff[:8], exp[frame], alt[frame])
    return frame


def test_a_wave_that_missed_the_planted_lane_would_differ(oracle_lib):
    planted_minus_zero_shows(oracle_lib)


# ---- C ----------------------------------------------------------------------------------------------------------------------------
def run_bounded_amount(lib, name, A, top, semantics, stage_jit, compiled):
    """Delay(Multiply(In0, 0.5), A) over two contiguous calls: the plan, the attained top and every frame.  compiled: the library
    can compile stage programs (the simulator interprets whatever FR_STAGE_JIT says)."""
    rows = pc.amount_rows()
    frames = pc.frames_of(pc.amount_values(A, rows, semantics))
    assert frames.max() == top, (name, semantics, int(frames.max()))                       # the amount ATTAINS the top
    g = pc.bounded_delay_graph(A)
    store, ref = sr.InputStore(), ldr.DenseForward(g, semantics)
    t = 0
    with Renderer(lib, mode="staged", options={"FR_STAGE_JIT": stage_jit}, semantics=semantics) as r:
        g.install(r)
        for n in pc.AMOUNT_CALLS:
            call = [row[t:t + n] for row in rows]
            got = r.fill_buffer(1, t, t + n, call)
            store.call(t, call)
            plan = r.plan()
            assert plan["pull_rows"] == 0 and plan["max_lookback"] >= top, (name, plan["pull_rows"], plan["max_lookback"])
            if compiled:
                assert plan["stage_jit"] == (stage_jit == "force"), (name, plan["stage_jit"])
            msg = ldr.first_diff(got, ref(store, t, t + n), f"{name} {semantics} FR_STAGE_JIT={stage_jit} [{t}, {t + n})")
            assert not msg, msg
            t += n
    # (the deepest reads happened: some frame past `top` read exactly `top` frames back)
    assert (frames[top:] == top).any()


@pytest.mark.parametrize("stage_jit", ["0", "force"])
@pytest.mark.parametrize("semantics", pc.pp.SEMANTICS)
@pytest.mark.parametrize("name,A,top", pc.BOUNDED_AMOUNTS, ids=[b[0] for b in pc.BOUNDED_AMOUNTS])
def test_bounded_amounts_reach_their_top(sim, name, A, top, semantics, stage_jit):
    run_bounded_amount(sim, name, A, top, semantics, stage_jit, compiled=False)


def run_dyn_loop(lib):
    """The loop whose Delay amount reaches its lower bound: refused unclamped (NaN for In1 = inf), a sweep plan clamped."""
    rows = pc.dyn_loop_rows()
    n = len(rows[0])
    with Renderer(lib, mode="staged", options=pc.LOOP_DYN) as r:
        pc.dyn_loop_graph(clamped=False).install(r)
        with pytest.raises(RenderError) as ei:
            r.fill_buffer(1, 0, n, rows)
        assert ei.value.status == FR_ERR_CYCLE, str(ei.value)
    g = pc.dyn_loop_graph()
    m = pc.pp.reference("Modulo", rows[1], np.float32(5.0))
    amount = pc.pp.reference("Sum2", np.float32(3.0), pc.pp.reference("Minimum", np.float32(5.0), m))
    assert pc.frames_of(amount).min() == 3 and pc.frames_of(amount).max() == 8 and not np.isnan(amount).any()
    store = sr.InputStore()
    store.call(0, rows)
    exp = ldr.DenseForward(g)(store, 0, n)
    with Renderer(lib, mode="staged", options=pc.LOOP_DYN) as r:
        g.install(r)
        got = r.fill_buffer(1, 0, n, rows)
        plan = r.plan()
    ld = plan["loop_dyn"]
    # the proven lower bound in frames: floor of the widened 3 + 0, at most the 3 frames the amount really reaches
    assert plan["feedback"] and plan["pull_rows"] == 0 and ld["sweep"] == 2 and 1 <= ld["frames"], ld
    assert [l["variant"] for l in plan["stage_launches"]] == ["stage_sweep_kernel/feedback+sweep"], plan["stage_launches"]
    msg = ldr.first_diff(got, exp, "a loop whose amount reaches its lower bound")
    assert not msg, msg
    assert np.isfinite(exp).all() and (exp != 0).sum() > n // 2


def test_a_loop_whose_amount_reaches_its_lower_bound(sim):
    run_dyn_loop(sim)


# ---- D: observed hulls (the drivers; on the simulator the reduction is the engine's host loop, on the MI355X input_range_kernel) ----
ENTRIES = ("device", "device_dense")


def spike_case(lib, oracle_lib, L, pos, value, entry, semantics="reference", options=None):
    """A fresh renderer, one call of L frames whose amount row is +0 but for `value` at `pos`: the plan after the call.  Every
    frame is compared with the oracle (Pair.call)."""
    # (a first call stores at most n_slots * n_times rows: a one-frame call needs two output rows to keep its amount row)
    tree = pc.observed_delay_tree(2 if L == 1 else 1)
    pair = Pair(lib, oracle_lib, tree, options=dict(pc.OBSERVED, **(options or {})), entry=entry, semantics=semantics)
    try:
        return pair.call(0, L, [pc.source_row(L), pc.spike_row(L, pos, value)], f"L={L} spike {value} at {pos} ({entry}, {semantics})")
    finally:
        pair.close()


def run_spike_edges(lib, oracle_lib, L, options=None):
    n = 0
    for pos in pc.spike_positions(L):
        for entry in ENTRIES:
            pl = spike_case(lib, oracle_lib, L, pos, 5.0, entry, options=options)
            assert pl["observed_lookback"] == 8 and pl["pull_rows"] == 0 and pl["observed_delays"] >= 1 and pl["range_launches"] > 0, (L, pos, entry, pl["observed_lookback"], pl["pull_rows"])
            n += 1
    return n


def run_negative_extreme(lib, oracle_lib, options=None):
    for pos in pc.spike_positions(257):
        pl = spike_case(lib, oracle_lib, 257, pos, -5.0, ENTRIES[pos % 2], options=options)
        assert pl["observed_lookback"] == 1 and pl["pull_rows"] == 0 and pl["range_launches"] > 0, (pos, pl["observed_lookback"], pl["pull_rows"])


def run_flags_at_the_last_element(lib, oracle_lib, options=None):
    L = pc.RANGE_BLOCK + 1
    for semantics in pc.pp.SEMANTICS:
        pl = spike_case(lib, oracle_lib, L, L - 1, np.inf, "device", semantics, options)
        assert pl["pull_rows"] > 0 and pl["observed_delays"] == 0, (semantics, pl["pull_rows"])           # +inf: no bound, refused
        for value in (np.nan, -np.inf):
            pl = spike_case(lib, oracle_lib, L, L - 1, value, "device", semantics, options)
            assert pl["pull_rows"] == 0 and pl["observed_delays"] == 1 and pl["observed_lookback"] == 1, (semantics, value, pl["pull_rows"])


N_SLOTS_33 = pc.RANGE_MAX_ROWS + 1


def run_33_slots(lib, oracle_lib, options=None):
    """33 observed amounts: a first call of +0 rows makes the plan that observes the 33 slots; the second call's rows -- of
    different lengths, row j with its spike 2^(j mod 5) at position j -- are reduced in two launches (32 rows and 1)."""
    pair = Pair(lib, oracle_lib, pc.observed_delay_tree(N_SLOTS_33), options=dict(pc.OBSERVED, **(options or {})), entry="device")
    try:
        T0, T1 = 64, 200 + 7 * N_SLOTS_33
        p0 = pair.call(0, T0, [pc.source_row(T0)] + [np.zeros(T0, np.float32)] * N_SLOTS_33, "33 slots, rows of +0")
        assert p0["pull_rows"] == 0 and p0["observed_delays"] == N_SLOTS_33 and p0["observed_lookback"] == 1, p0
        rows = [np.arange(T0 + 1, T0 + T1 + 1, dtype=np.float32)]
        for j in range(N_SLOTS_33):
            rows.append(pc.spike_row(200 + 7 * j, j, 2.0 ** (j % 5)))
        assert len({len(r) for r in rows}) == N_SLOTS_33 + 1
        p1 = pair.call(T0, T0 + T1, rows, "33 slots, spikes")
    finally:
        pair.close()
    assert p1["range_launches"] - p0["range_launches"] == 2, (p0["range_launches"], p1["range_launches"])
    assert p1["pull_rows"] == 0 and p1["observed_delays"] == N_SLOTS_33 and p1["observed_lookback"] == 16, p1


def run_rebuild(lib, oracle_lib, options=None, spike_at=pc.RANGE_BLOCK):
    """The first plan observes nothing (the Delay has no output edge yet); a 20 000-frame row with its spike at 16384 is stored; the
    edit adds the edge; observed_range reduces the stored history (two blocks) when the new plan asks for the slot."""
    L, T = 20000, 256
    g = synth.GraphArrays()
    src = g.binop(synth.K_MUL, synth.IN(0), synth.C(np.array([0.5], np.float32)), 1)
    dl = g.nodes(synth.K_DELAY, 1)
    g.edge(src, dl, 0, 0)
    g.edge(0, dl, 1, 1)
    g.edge(src, 0, 0, 0)
    tree = g.finish(2)
    pair = Pair(lib, oracle_lib, tree, options=dict(pc.OBSERVED, **(options or {})), entry="device")
    try:
        p0 = pair.call(0, L, [pc.source_row(L), pc.spike_row(L, spike_at, 5.0)], "before the edit")
        assert p0["observed_delays"] == 0 and p0["range_launches"] == 0, p0
        for r in (pair.r, pair.ref):
            r.on_add_edge(int(dl[0]), 0, 0, 1)
        amount = np.zeros(T, np.float32)
        amount[T // 2:] = 2.0                 # (the call's own rows stay below the stored spike: alone they would plan 4 frames)
        amount[7] = 3.0
        p1 = pair.call(L, L + T, [np.arange(L + 1, L + T + 1, dtype=np.float32), amount], "after the edit")
    finally:
        pair.close()
    assert p1["pull_rows"] == 0 and p1["observed_delays"] == 1 and p1["observed_lookback"] == 8 and p1["range_launches"] >= 1, p1


SIM_JIT_OFF = {"FR_STAGE_JIT": "0"}
REBUILD_SPIKES = (pc.RANGE_BLOCK, pc.RANGE_BLOCK + 300)      # the second block's first element, and one of its second wave's


@pytest.mark.parametrize("L", [L for L in pc.SPIKE_LENGTHS if L <= 257])
def test_observed_hull_edges_host_logic(sim, oracle_lib, L):
    assert run_spike_edges(sim, oracle_lib, L, SIM_JIT_OFF) == 2 * len(pc.spike_positions(L))


def test_observed_hull_negative_flags_slots_and_rebuild_host_logic(sim, oracle_lib):
    run_negative_extreme(sim, oracle_lib, SIM_JIT_OFF)
    run_flags_at_the_last_element(sim, oracle_lib, SIM_JIT_OFF)
    run_33_slots(sim, oracle_lib, SIM_JIT_OFF)
    for spike_at in REBUILD_SPIKES:
        run_rebuild(sim, oracle_lib, SIM_JIT_OFF, spike_at)
