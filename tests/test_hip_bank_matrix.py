"""Every bank kernel instance the launch rule can pick (tests/bank_variants.py), on the MI355X, against the dense f32
reference (tests/bank_reference.py) on EVERY output sample, bit for bit (NaN == NaN).

Per case: the renderer gets the case's options, and each call asserts from fr_plan_json that it ran the case's variant.  The
voices hold silent +0 and -0 voices, a voice with one zero amplitude, and a voice whose partials all lie beyond 2^23 cycles at
the ramp's offset (every leaf an exact zero: the zero-sign repair on every frame).  Calls: a ramp at 2^20 plus a ragged start,
T frames (not a multiple of 64 F); a hostile row of the same length -- a wave of tiny and fractional negative times (the
general path, where fract and fmod differ near zero) and a wave of NaN, +-inf, 1e30, 3e38, 2^32, 8e9, -0 and subnormals;
then a call of another length T2, reusing workspace, tickets and row-completion counters.  The same variant then renders a
tree whose group has one voice of negative w (the host clears fast_ok: every wave on the general path).  The C++ oracle is
sought at the first and last frame of each call, frames 63 and 64, the first frame of the last tile and a tile boundary (the
trees have no Delay, so a seek is exact), which pins the reference to it on the GPU's very rows."""
import numpy as np
import pytest

import bank_reference
import bank_variants
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu

OFFSET = (1 << 20) + 37
HOSTILE_NEG = np.array([-1e-9, -1e-30, -1e-45, -1e-20, -0.3, -2.5, -1e-7, -0.75, -3e-39, -1.5e-8, -0.001, -17.25], np.float32)
HOSTILE_ODD = np.array([np.nan, np.inf, -np.inf, 1e30, 3e38, 4294967296.0, 8e9, -0.0, 1e-45, 3e-39, 0.625, 2.5e-7], np.float32)


def voices(V, P, seed, negative_voice=False):
    """w, amp [V, P].  The first voices are the special ones, in this order: a sounding voice with one zero amplitude, a voice
    whose t * w all lie beyond 2^23 at the ramp's offset (every leaf an exact zero), a silent -0 voice, a silent +0 voice, a
    voice of mixed +0 / -0 / sounding amplitudes; the rest are regular (fundamentals repeat, so none lies wholly beyond 2^23)."""
    p = synth.voice_params(V, P, seed=seed, wrap=24)
    rng = np.random.default_rng(seed)
    w = (p["w"] * np.float32(0.25) + (rng.random((V, P)) * 1e-3).astype(np.float32)).astype(np.float32)   # (distinct partials)
    amp = p["amp"].copy()
    k = np.arange(P)
    special = [
        lambda v: amp.__setitem__((v, P // 3), 0.0),
        lambda v: w.__setitem__(v, (8.0 + k * 0.5).astype(np.float32)),
        lambda v: amp.__setitem__(v, -0.0),
        lambda v: amp.__setitem__(v, 0.0),
        lambda v: amp.__setitem__(v, np.where(k % 5 == 0, 0.0, np.where(k % 5 == 1, -0.0, amp[v])).astype(np.float32)),
    ]
    for v, f in enumerate(special[:V]):
        f(v)
    if negative_voice:
        w[V - 1] = -w[V - 1]
    return w, amp.astype(np.float32)


def hostile_row(idx, T, F):
    """The ramp with a wave of negative times and a later wave of the other hostile values."""
    row = synth.time_ramp(idx, idx + T)
    if T <= 2:
        return np.array([-1e-30, np.nan][:T], np.float32)
    a = min(64 * F + 5, T - len(HOSTILE_NEG))          # (a wave of its own where the call has two)
    row[a:a + len(HOSTILE_NEG)] = HOSTILE_NEG
    b = T - len(HOSTILE_ODD) - 1
    if b >= a + len(HOSTILE_NEG):
        row[b:b + len(HOSTILE_ODD)] = HOSTILE_ODD
    return row


class Entry:
    """fill_buffer (host) or fill_buffer_device (device) of one renderer."""

    def __init__(self, r, kind):
        self.r, self.kind = r, kind

    def __call__(self, V, idx, row):
        T = len(row)
        if self.kind == "host":
            return self.r.fill_buffer(V, idx, idx + T, [row])
        import torch
        d_row = torch.from_numpy(np.ascontiguousarray(row)).cuda()
        d_out = torch.full((V, T), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        self.r.fill_buffer_device(d_out.data_ptr(), V, T, idx, d_row.data_ptr(), [0, T], 0)
        torch.cuda.synchronize()
        return d_out.cpu().numpy()


def workgroups(b):
    """The workgroups of a reported launch (kernels.hip launch_bank, launch_gbank; jit.cpp launch_jit_bank)."""
    F, v, vpw = b["frames_per_lane"], b["voices"], b["voices_per_wave"]
    tiles = -(-b["frames"] // (64 * F))
    if b["small_call"] == 1:
        return v << (b["partials"].bit_length() - 1 - 8)
    if vpw:
        return tiles * -(-v // (4 * vpw))
    if b["kernel"] == "gbank":
        return tiles * v
    if b["kernel"] == "jit_bank":
        return (tiles * v) << b["pieces_log2"]
    return (tiles * v) << (b["partials"].bit_length() - 1 - b["chunk_log2"])


def seek_frames(T, F):
    tile = 64 * F
    return sorted({c for c in (0, T - 1, 63, 64, ((T - 1) // tile) * tile, tile - 1, tile, 2 * tile) if 0 <= c < T})


def check_call(case, hip, entry, ref, w, amp, idx, row, what):
    V = case["V"]
    got = entry(V, idx, row)
    launches = hip.plan()["bank_launches"]
    variants = [b["variant"] for b in launches]
    b = max(launches, key=lambda x: x["voices"]) if launches else {}
    # (generated kernels: voices whose leaves fold to other literals -- a zero amplitude -- are compiled as groups of their
    #  own; every group runs a generated kernel, and the case's variant is the main group's)
    if case["kind"] == "jit":
        assert b.get("variant") == case["key"] and all(v.startswith("jit_bank") for v in variants), f"{what}: ran {launches}"
    else:
        assert variants == [case["key"]], f"{what}: ran {variants}, expected {case['key']}: {launches}"
    assert sum(x["voices"] for x in launches) == V and b["frames"] == len(row), (what, launches)
    assert b["publishes_rows"] == ("flags" in case["key"]), (what, b)
    assert b["leaf_variant"] == int(case["options"].get("FR_BANK_LEAF", 1)), (what, b)
    if what == "ramp":   # (the XCD block remap is taken exactly when the count is a multiple of 8)
        assert (workgroups(b) % 8 == 0) == case["xcd"], (what, workgroups(b), b)
    F = b["frames_per_lane"]
    exp = bank_reference.render_bank(w, amp, row)
    msg = bank_reference.first_diff(got, exp, f"{case['key']} {what} (call at {idx}, {len(row)} frames)")
    assert not msg, msg
    for c in seek_frames(len(row), F):
        o = ref.fill_buffer(V, idx + c, idx + c + 1, [row[c:c + 1]])
        msg = bank_reference.first_diff(exp[:, c:c + 1], o, f"{case['key']} {what}: dense reference vs oracle at frame {c}")
        assert not msg, msg


@pytest.mark.parametrize("case", bank_variants.CASES, ids=[c["key"] for c in bank_variants.CASES])
def test_bank_variant_against_dense_reference(hip_lib, oracle_lib, case):
    V, P, T, T2 = case["V"], case["P"], case["T"], case["T2"]
    for negative in (False, True):
        w, amp = voices(V, P, seed=P * 7 + V, negative_voice=negative)
        tree = bank_reference.bank_tree(w, amp)
        with Renderer(hip_lib, options=case["options"]) as hip, Renderer(oracle_lib) as ref:
            synth.install(hip, tree)
            synth.install(ref, tree)
            entry = Entry(hip, case["entry"])
            F = int(case["options"].get("FR_BANK_F", 1))
            calls = [("ramp", OFFSET, synth.time_ramp(OFFSET, OFFSET + T)),
                     ("hostile row", OFFSET + T, hostile_row(OFFSET + T, T, F))]
            if not negative:
                calls.append(("second length", OFFSET + 2 * T, synth.time_ramp(OFFSET + 2 * T, OFFSET + 2 * T + T2)))
            for what, idx, row in calls:
                check_call(case, hip, entry, ref, w, amp, idx, row, ("negative-w tree, " if negative else "") + what)
            assert hip.plan()["pull_rows"] == 0
