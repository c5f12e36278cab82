"""The bank kernel instances on the CPU: the dense reference (tests/bank_reference.py) pinned bit for bit to the C++ oracle
on the inputs where kernels go wrong, and the GPU case table (tests/bank_variants.py) checked against every key the launch
rule can produce (tests/cpp/bankplan_sweep.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import bank_reference
import bank_variants
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
SWEEP_SRC = os.path.join(ROOT, "tests", "cpp", "bankplan_sweep.cpp")
SWEEP_BIN = os.path.join(ROOT, "tests", "cpp", "_build", "bankplan_sweep")

HOSTILE = np.array([-3.25, np.nan, np.inf, -np.inf, 1e30, 3e38, 4294967296.0, 8e9, -0.0, 1e-45, -1e-45, 0.375, -1e-30, 2.5, -0.6, 0.0,
                    1e-30, 16777217.0, 1048576.5, -7.0], np.float32)


# ---- the dense reference against the C++ oracle ---------------------------------------------------------------------------
def _params(V, P, seed):
    """Voices that exercise every sign case: regular partials, negative w, silent +0 / -0 / mixed-zero voices, one zero amplitude."""
    rng = np.random.default_rng(seed)
    w = (rng.random((V, P)) * 0.05).astype(np.float32)
    amp = (1.0 / np.arange(1, P + 1, dtype=np.float32))[None, :].repeat(V, 0)
    w[0] = -w[0]                                               # negative w: the fmod path and its fix-up
    if V > 1:
        amp[1] = 0.0                                           # silent, +0
    if V > 2:
        amp[2] = -0.0                                          # silent, -0
    if V > 3:
        amp[3, ::2] = 0.0                                      # mixed zeros
        amp[3, 1::2] = -0.0
    if V > 4:
        amp[4, P // 2] = 0.0                                   # one zero amplitude in a sounding voice
        w[4, ::3] = -w[4, ::3]
    if V > 5:
        w[5] = (np.arange(P) % 8 + 1).astype(np.float32) / 16  # t * w integral every 16 frames: exact zero leaves
    return w, amp.astype(np.float32)


@pytest.mark.parametrize("P", [1, 3, 7, 24, 100, 256, 1000])
def test_reference_matches_oracle(oracle_lib, P):
    """Every frame, bit for bit: a ramp at a large offset, the hostile time values (negative, NaN, +-inf, 1e30, 3e38, 2^32,
    8e9, -0, subnormal, fractional), negative ramps and random mixed-sign rows; negative w; silent voices of +0, -0 and mixed
    zero amplitudes; a zero amplitude among sounding ones; non-power-of-two partial counts (odd carries)."""
    V = 6
    w, amp = _params(V, P, seed=P)
    tree = bank_reference.bank_tree(w, amp)
    rng = np.random.default_rng(P + 1)
    rows = [
        np.arange(1 << 20, (1 << 20) + 40, dtype=np.float32),
        HOSTILE,
        -np.arange(0, 40, dtype=np.float32) * np.float32(0.37),
        (rng.normal(size=40) * 1e4).astype(np.float32),
        np.arange(0, 48, dtype=np.float32),
    ]
    with Renderer(oracle_lib) as ref:
        synth.install(ref, tree)
        idx = 0
        for i, row in enumerate(rows):
            exp = ref.fill_buffer(V, idx, idx + len(row), [row])
            got = bank_reference.render_bank(w, amp, row, budget=1 << 12)
            msg = bank_reference.first_diff(got, exp, f"P={P} row {i}")
            assert not msg, msg
            idx += len(row)
    # a row through the slicing: voices and frames cut into many pieces give the same bits as one piece
    t = np.concatenate([HOSTILE, np.arange(5000, 5077, dtype=np.float32)])
    assert not bank_reference.first_diff(bank_reference.render_bank(w, amp, t, budget=P * 7), bank_reference.render_bank(w, amp, t, budget=1 << 24))


def test_reference_detects_a_wrong_zero_sign():
    """The comparison tells -0 from +0 and matches NaN with NaN."""
    a = np.array([[0.0, np.nan, 1.0]], np.float32)
    b = np.array([[-0.0, np.nan, 1.0]], np.float32)
    assert "voice 0, frame 0" in bank_reference.first_diff(a, b)
    assert bank_reference.first_diff(a, a.copy()) == ""


# ---- the launch rule's reachable instances ---------------------------------------------------------------------------------
def _sweep_bin():
    deps = [SWEEP_SRC] + [os.path.join(CSRC, f) for f in ("bankplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp")]
    if not os.path.exists(SWEEP_BIN) or os.path.getmtime(SWEEP_BIN) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SWEEP_BIN), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", SWEEP_BIN, SWEEP_SRC], check=True)
    return SWEEP_BIN


def query(lines):
    """tests/cpp/bankplan_sweep.cpp --query: (key, workgroups, voices per wave) of each launch."""
    p = subprocess.run([_sweep_bin(), "--query"], input="".join(x + "\n" for x in lines), capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr
    return [(k, int(n), int(vpw)) for k, n, vpw in (ln.split() for ln in p.stdout.splitlines())]


def case_launch(case, n_times):
    """The query line of a case's call: its group as the engine plans it, and its options as BankTuning."""
    o = case["options"]
    P = case["P"]
    kind = {"balanced": 0, "jit": 1, "general": 2}[case["kind"]]
    log2_p = 0 if kind == 2 else P.bit_length() - 1
    row_flags = int(case["entry"] == "host" and case["V"] * n_times * 4 >= 256 << 10)
    # (generated kernels: the two silent voices of tests/test_hip_bank_matrix.py, all of whose amplitudes are literal zeros, are
    #  compiled as groups of their own; the case's variant is that of the main group, the other voices)
    voices = case["V"] - 2 if kind == 1 else case["V"]
    fields = [kind, log2_p, voices, P if kind == 2 else 0, 0, int(kind == 1), n_times, 0, row_flags,
              int(o.get("FR_BANK_SHORT", "1") != "0"), o.get("FR_SHORT_PAIRS", 1000), o.get("FR_SHORT_WGS", 0), o.get("FR_SHORT_NW", 0),
              o.get("FR_BANK_F", 0), o.get("FR_BANK_NW", 0), int(o.get("FR_BANK_MULTI", "1") != "0"), o.get("FR_BANK_LEAF", 1),
              int(o.get("FR_JIT_CHUNKS", "1") != "0"), o.get("FR_JIT_CHUNK_TARGET", 0)]
    return " ".join(str(f) for f in fields)


def test_sweep_reaches_exactly_the_table():
    """The set of keys the rule can produce over its whole grid equals the GPU case table's keys, and none of the
    instantiations listed as unreachable is among them.  A new variant without a case fails here."""
    p = subprocess.run([_sweep_bin()], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    reached = {ln.split("\t")[0] for ln in lines[:-1]}
    assert lines[-1].startswith(f"{len(reached)} keys"), lines[-1]
    table = [c["key"] for c in bank_variants.CASES]
    assert len(table) == len(set(table)), "a key has two cases"
    assert reached == set(table), (f"reachable without a case: {sorted(reached - set(table))}; "
                                   f"cases for keys the rule never picks: {sorted(set(table) - reached)}")
    assert not reached & set(bank_variants.UNREACHABLE), sorted(reached & set(bank_variants.UNREACHABLE))
    print("reachable bank variants:", ", ".join(sorted(reached)))


def test_every_case_reaches_its_key():
    """Each GPU case's shape and options reach the key it is named after on both call lengths (the GPU test asserts the
    same from fr_plan_json); each family whose kernels remap workgroups onto XCDs has a case with a workgroup count that is
    a multiple of 8 and one with a count that is not, as the table declares."""
    lines = [case_launch(c, T) for c in bank_variants.CASES for T in (c["T"], c["T2"])]
    got = query(lines)
    for i, c in enumerate(bank_variants.CASES):
        (k1, n1, vpw), (k2, _, _) = got[2 * i], got[2 * i + 1]
        assert k1 == c["key"] and k2 == c["key"], (c, k1, k2)
        assert (n1 % 8 == 0) == c["xcd"], (c["key"], n1)
        assert 2 <= c["T"] or c["key"].startswith("bank_small_kernel"), c
        assert c["T"] != c["T2"], c
        if vpw:   # whole voices per wave: a voice count that leaves the last workgroup's waves partly empty
            assert c["V"] % (4 * vpw), (c, vpw)
    for fam in bank_variants.XCD_FAMILIES:
        seen = {c["xcd"] for c in bank_variants.CASES if c["key"].startswith(fam)}
        assert seen == {True, False}, (fam, seen)


def test_unreachable_instantiations_exist():
    """The unreachable list names instantiations that kernels.hip really compiles (so the list is not stale)."""
    src = open(os.path.join(CSRC, "kernels.hip")).read()
    for key in bank_variants.UNREACHABLE:
        name, args = key.rstrip(">").split("<")
        a = [x.lstrip("FMNW") for x in args.split(",")]
        # launch_bank_f instantiates bank_kernel<F, MODE, NW> for its F; launch_bank names bank_multi_kernel<F, MODE> in full
        inst = f"bank_kernel<F, {a[1]}, {a[2]}>" if name == "bank_kernel" else f"{name}<{a[0]}, {a[1]}>"
        assert inst in src, key
    assert "case 1: return launch_bank_f<1>" in src and "case 2: return launch_bank_f<2>" in src and "case 4: return launch_bank_f<4>" in src
