"""Every launch form at sample indices around 2^24, 2^31, 2^32, 2^40 and 2^62, on the MI355X: the table of tests/abs_index.py.

A case's sequence -- a seek to B - 100, contiguous calls (blocks) that cross B in the middle of a call and of a 64-frame
group, one frame, a seek forward to B + 5003, a seek back across B to B - 40 and, up to 2^40, a far seek to B + 2^33 + 69 --
runs at the high frames, and EVERY sample must equal the dense reference of the sequence's low twin bit for bit, NaN equal to
NaN, +0 unequal to -0 (the shift rule; tests/test_abs_index.py proves it per case and base against the C++ oracle rendered at
the high frames, and proves that at least half of every expected row is finite and non-zero).  In addition the oracle is sought
here at the high index itself at the first and last frame of each call, at B - 1, B, B + 1 and at B + d for the case's delays.

One test per case loops over 2^24, 2^32 and 2^62; one test per family (pull, stage interpreter, compiled stage, bank to rings,
stream) takes 2^31 and 2^40.  Each call asserts the kernel or key that ran from fr_plan_json, a stream after its first block.
A stream's references are rendered before fr_stream_begin and compared after fr_stream_end; the X.IDLE options bound what a
block that is not answered costs.  profiles/abs_index.txt has the durations."""
import pytest

import abs_index as A
import stage_reference as sr
import stream_matrix as X
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in list(X.ALL) + ["FR_LOOP_TILES", "FR_STREAM_IDLE_MS", "FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"]:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def run_stream(r, c, blocks):
    """One stream of the open renderer `r`: fr_stream_begin, every block through fr_stream_block_rows, fr_stream_end."""
    r.stream_begin(c["n_rows"])
    out = []
    for k, (idx, T, rows) in enumerate(blocks):
        out.append(r.stream_block_rows(idx, rows, n_times=T))
        if k == 0:
            c["check"](r.plan(), k, T)
    r.stream_end()
    return out


def run_case(hip_lib, oracle_lib, c, bases):
    name = c["name"]
    low, expected = A.low_twin(name)
    highs = [A.rebase(low, B, c["s0"]) for B in bases]
    wanted = [A.special_frames(h, B, c["delays"]) for h, B in zip(highs, bases)]
    oracle = [A.oracle_at(oracle_lib, c, h, w) for h, w in zip(highs, wanted)]       # before any stream opens
    got = []
    if c["kind"] == "stream":
        with Renderer(hip_lib, semantics=c["semantics"], options=dict(c["options"], **X.IDLE)) as r:
            c["install"](r)
            for high in highs:
                got.append(run_stream(r, c, high))
    elif c["kind"] == "mixed":
        for high in highs:
            got.append(A.run_mixed(hip_lib, c, high, options=dict(c["options"], **X.IDLE)))
    else:
        for high in highs:                                                            # a renderer per base: an edit is made once
            got.append(A.run_calls(hip_lib, c, high, after=c["check"]))
    n = 0
    for B, high, out, at in zip(bases, highs, got, oracle):
        assert len(out) == len(high) and (len(high) == len(low)) == (B <= A.FAR_MAX_BASE)
        for k, ((idx, T, _), g, e) in enumerate(zip(high, out, expected)):
            msg = sr.first_diff(g, e, f"{name} at B = {B}: call {k} at frame {idx} = B{idx - B:+d} (T={T}) against the low twin's reference")
            assert not msg, msg
            n += T
        for (k, col), v in at.items():
            msg = sr.first_diff(g_col(out[k], col), v.reshape(-1, 1), f"{name} at B = {B}: frame {high[k][0] + col} (call {k}) against the oracle")
            assert not msg, msg
    print(f"{name}: {n} frames compared at {len(bases)} bases, {sum(len(a) for a in oracle)} of them with the oracle at the high index")


def g_col(a, col):
    return a[:, col:col + 1]


@pytest.mark.parametrize("name", [c["name"] for c in A.CASES])
def test_every_sample_at_2_24_2_32_and_2_62(hip_lib, oracle_lib, name):
    run_case(hip_lib, oracle_lib, A.case(name), A.EVERY_CASE)


@pytest.mark.parametrize("family", A.FAMILIES)
def test_a_case_of_every_family_at_2_31_and_2_40(hip_lib, oracle_lib, family):
    run_case(hip_lib, oracle_lib, A.case(A.FAMILY_CASE[family]), A.PER_FAMILY)


@pytest.mark.parametrize("stage_jit", ["0", "force"])
def test_a_feedback_plan_refuses_what_it_cannot_replay(hip_lib, stage_jit):
    """A seek to 2^28 + 1 is refused with FR_ERR_UNSUPPORTED and the frame's number; the renderer then serves a seek to frame 300,
    every sample equal to the dense reference."""
    A.feedback_refusal(hip_lib, {"FR_STAGE_JIT": stage_jit})
