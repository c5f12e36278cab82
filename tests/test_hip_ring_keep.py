"""FR_RING_KEEP on the GPU: the HIP library against the oracle and against itself with the option off, bit for bit, over
the sequences of tests/ring_keep_cases.py (tests/test_ring_keep_sim.py runs the same on the host-logic simulator)."""
import pytest

import ring_keep_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ("FR_RING_KEEP", "FR_TRACK_HISTORY", "FR_DELAY_OBSERVED", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("stage_jit", ["0", "force"])
def test_effects_chain_edits(hip_lib, oracle_lib, stage_jit):
    K.run_chain_sequence(hip_lib, oracle_lib, extra_options={"FR_STAGE_JIT": stage_jit})


@pytest.mark.timeout(900)
@pytest.mark.parametrize("d", [100, 1])
def test_comb_loops_are_not_replayed_for_edits_outside_them(hip_lib, oracle_lib, d):
    """Oracle, option off and option on on every call, the edits included (a short sequence: the oracle's recursion costs
    frame / d voice evaluations per frame)."""
    if d == 100:
        K.run_comb_sequence(hip_lib, oracle_lib, d, reach=2500, first=(100, 150, 250), step=400, after=(60, 40))
    else:
        K.run_comb_sequence(hip_lib, oracle_lib, d, reach=500, first=(100, 150, 250), step=100, after=(60, 40))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("d", [100, 1])
def test_comb_loops_at_frame_40000(hip_lib, d):
    """The same edits after 40 000 frames, the rings wrapped: option off against option on, every call."""
    K.run_comb_sequence(hip_lib, None, d)


def test_merged_loop(hip_lib, oracle_lib):
    K.run_merged_loop(hip_lib, oracle_lib)


@pytest.mark.parametrize("stage_jit", ["0", "force"])
def test_random_edits_between_calls(hip_lib, oracle_lib, stage_jit):
    assert K.run_random_edits(hip_lib, oracle_lib, range(0, 40), extra_options={"FR_STAGE_JIT": stage_jit}) == 0


@pytest.mark.timeout(900)
@pytest.mark.parametrize("stage_jit", ["0", "force"])
def test_feedback_graphs_edited_during_playback(hip_lib, oracle_lib, stage_jit):
    done, off, on = K.run_random_feedback_edits(hip_lib, oracle_lib, range(0, 80), extra_options={"FR_STAGE_JIT": stage_jit})
    assert done >= 40 and on == off and 10 * off <= done, (done, off, on)


@pytest.mark.parametrize("grow", [False, True])
@pytest.mark.parametrize("arrangement", sorted(K.MOVE_ARRANGEMENTS))
@pytest.mark.parametrize("rings", [1, 3, 64, 700])
def test_ring_move_kernel_through_the_engine(hip_lib, oracle_lib, rings, arrangement, grow):
    """1, 3, 64 and 700 rings moved by ring_move_kernel, renumbered at 1024 frames a ring and 1024 -> 4096, over spans that
    cross the wrap in the source only, in both, in neither, and over three segments with misaligned ends (700 rings: option off
    against option on; the oracle takes the smaller ones)."""
    K.run_moves(hip_lib, oracle_lib, rings, arrangement, grow)
