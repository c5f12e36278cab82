"""Per-renderer options (include/friendship_render_ext.h) on the MI355X: two renderers of one process that differ in an
option each launch by their own -- the short-call bank kernel, the FMA fold of generated leaves, compiled stage programs,
the streamed host path -- and render the same bits as each other and as the oracle.  fr_plan_json's "bank_launches"
shows which bank kernel the last call ran.  The option table itself is checked on the CPU (tests/test_options_sim.py)."""
import os

import numpy as np
import pytest

from kat_replay import same_bits
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu

BANK_SWITCHES = ["FR_BANK_SHORT", "FR_SHORT_PAIRS", "FR_SHORT_WGS", "FR_SHORT_NW", "FR_BANK_NW", "FR_BANK_F", "FR_BANK_MULTI",
                 "FR_BANK_LEAF", "FR_BANK_TEMPLATE", "FR_JIT", "FR_JIT_FMA", "FR_STAGE_JIT", "FR_HOST_STREAM", "FR_HOST_MAPPED",
                 "FR_HOST_SMALL_KB", "FR_JIT_CACHE"]


@pytest.fixture
def clean_env(monkeypatch):
    for name in BANK_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def kernels(r):
    return [b["kernel"] for b in r.plan()["bank_launches"]]


def oracle_frames(oracle_lib, tree, n_slots, frames):
    """The oracle's value of every slot at each frame (by seeking: the trees here have no Delay)."""
    with Renderer(oracle_lib) as ref:
        synth.install(ref, tree)
        return {c: ref.fill_buffer(n_slots, c, c + 1, [synth.time_ramp(c, c + 1)]) for c in frames}


def check_frames(out, idx, exp):
    for c, e in exp.items():
        if idx <= c < idx + out.shape[1]:
            assert same_bits(out[:, c - idx:c - idx + 1], e), f"frame {c}"


def test_short_call_kernel_per_renderer(hip_lib, oracle_lib, clean_env):
    """8 voices x 4096 partials.  Renderer A has the defaults, B FR_BANK_SHORT=0, made only after A has launched the
    short-call kernel (a process-wide switch read once would give B A's choice).  At 64 frames A takes the short-call kernel
    and B the time-major one; at 4800 frames B still never takes it.  Calls interleave; every output is the same bits on
    both and the oracle's on sampled frames."""
    V, P = 8, 4096
    tree = synth.additive_tree(n_voices=V, n_partials=P, seed=0x5EED0101)
    calls = [(0, 64), (64, 4800), (4864, 64)]
    exp = oracle_frames(oracle_lib, tree, V, [0, 31, 63, 64, 1000, 4000, 4863, 4864, 4927])
    with Renderer(hip_lib) as a:
        synth.install(a, tree)
        first = a.fill_buffer(V, 0, 64, [synth.time_ramp(0, 64)])
        assert kernels(a) == ["bank_short_kernel"], a.plan()["bank_launches"]
        with Renderer(hip_lib, options={"FR_BANK_SHORT": "0"}) as b:
            assert b.options()["FR_BANK_SHORT"] == {"value": "0", "source": "option"}
            assert a.options()["FR_BANK_SHORT"] == {"value": "1", "source": "default"}
            synth.install(b, tree)
            for i, (idx, T) in enumerate(calls):
                row = synth.time_ramp(idx, idx + T)
                oa = first if i == 0 else a.fill_buffer(V, idx, idx + T, [row])
                ka = kernels(a)
                ob = b.fill_buffer(V, idx, idx + T, [row])
                kb = kernels(b)
                assert "bank_short_kernel" not in kb and kb, (idx, T, b.plan()["bank_launches"])
                if T == 64:
                    assert ka == ["bank_short_kernel"] and kb == ["bank_kernel"], (ka, kb)
                    launch = b.plan()["bank_launches"][0]
                    assert launch["voices"] == V and launch["partials"] == P and launch["frames"] == T
                assert same_bits(oa, ob), (idx, T)
                check_frames(oa, idx, exp)


def test_short_call_kernel_follows_the_environment_at_creation(hip_lib, oracle_lib, clean_env):
    """The same through the environment: FR_BANK_SHORT=0 set after A launched the short-call kernel applies to a renderer
    created afterwards, and not to A."""
    V, P = 8, 4096
    tree = synth.additive_tree(n_voices=V, n_partials=P, seed=0x5EED0102)
    exp = oracle_frames(oracle_lib, tree, V, [0, 63, 64, 127])
    with Renderer(hip_lib) as a:
        synth.install(a, tree)
        oa = [a.fill_buffer(V, 0, 64, [synth.time_ramp(0, 64)])]
        assert kernels(a) == ["bank_short_kernel"]
        clean_env.setenv("FR_BANK_SHORT", "0")
        with Renderer(hip_lib) as c:
            assert c.options()["FR_BANK_SHORT"] == {"value": "0", "source": "env"}
            synth.install(c, tree)
            oc = [c.fill_buffer(V, 0, 64, [synth.time_ramp(0, 64)])]
            assert kernels(c) == ["bank_kernel"]
            oa.append(a.fill_buffer(V, 64, 128, [synth.time_ramp(64, 128)]))
            assert kernels(a) == ["bank_short_kernel"]
            oc.append(c.fill_buffer(V, 64, 128, [synth.time_ramp(64, 128)]))
            assert kernels(c) == ["bank_kernel"]
    for i, idx in enumerate((0, 64)):
        assert same_bits(oa[i], oc[i])
        check_frames(oa[i], idx, exp)


def triangle_tree(V, P, seed):
    p = synth.voice_params(V, P, seed=seed)
    g = synth.GraphArrays()
    leaves = synth.triangle_leaves(g, p["w"], p["amp"]).reshape(V, P)
    g.edge(synth.sum_tree(g, leaves), 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def test_jit_fma_per_renderer(hip_lib, oracle_lib, clean_env, tmp_path):
    """Triangle partials, compiled with hipRTC in the call.  With a kernel cache on disk (process-wide): A (defaults)
    compiles and stores its kernel; B (FR_JIT_FMA=0) generates other source, so it compiles its own instead of loading A's;
    C (defaults) loads A's.  All three render the same bits, the oracle's."""
    cache = tmp_path / "jit"
    cache.mkdir(mode=0o700)
    os.chmod(cache, 0o700)
    clean_env.setenv("FR_JIT_CACHE", str(cache))
    V, P, T = 4, 256, 512
    tree = triangle_tree(V, P, seed=0x5EED0103)
    exp = oracle_frames(oracle_lib, tree, V, [0, 1, 255, 511])
    outs, plans = {}, {}
    for name, opts in (("a", None), ("b", {"FR_JIT_FMA": "0"}), ("c", None)):
        with Renderer(hip_lib, options=opts) as r:
            synth.install(r, tree)
            outs[name] = r.fill_buffer(V, 0, T, [synth.time_ramp(0, T)])
            plans[name] = r.plan()
            assert r.options()["FR_JIT_FMA"]["value"] == ("0" if name == "b" else "1")
        assert [b["jit"] for b in plans[name]["banks"]] == [True], plans[name]
        assert [x["kernel"] for x in plans[name]["bank_launches"]] == ["jit_bank"], plans[name]
        files = sorted(cache.glob("fr_*.jitbin"))
        assert len(files) == {"a": 1, "b": 2, "c": 2}[name], files
    assert plans["a"]["jit_disk_hits"] == 0 and plans["a"]["jit_kernels_compiled"] == 1
    assert plans["b"]["jit_disk_hits"] == 0 and plans["b"]["jit_kernels_compiled"] == 1   # a hit would be A's code object
    assert plans["c"]["jit_disk_hits"] == 1
    for name in "abc":
        check_frames(outs[name], 0, exp)
        assert same_bits(outs[name], outs["a"]), name


def test_stage_jit_per_renderer(hip_lib, oracle_lib, clean_env):
    """FR_STAGE_JIT=force against 0 on a plan with stage programs: one renderer runs them compiled, the other interpreted,
    calls interleaved, same bits as each other and as the oracle."""
    V = 3
    tree = synth.effects_tree(V, 32, taps=3, base_delay=50.0)
    calls = [(0, 128), (128, 64), (192, 300)]
    with Renderer(oracle_lib) as ref:
        synth.install(ref, tree)
        exp = [ref.fill_buffer(V, idx, idx + T, [synth.time_ramp(idx, idx + T)]) for idx, T in calls]
    with Renderer(hip_lib, options={"FR_STAGE_JIT": "force"}) as a, Renderer(hip_lib, options={"FR_STAGE_JIT": "0"}) as b:
        synth.install(a, tree)
        synth.install(b, tree)
        for (idx, T), e in zip(calls, exp):
            row = synth.time_ramp(idx, idx + T)
            oa = a.fill_buffer(V, idx, idx + T, [row])
            ob = b.fill_buffer(V, idx, idx + T, [row])
            assert b.plan()["stage_jit"] is False
            assert same_bits(oa, e) and same_bits(ob, e), (idx, T)
        assert a.plan()["stage_jit"] is True and a.plan()["stage_programs"] + a.plan()["fused_programs"] > 0


def test_host_stream_per_renderer(hip_lib, clean_env):
    """FR_HOST_STREAM=0 on one renderer: host-buffer results of >= 256 KB leave in one copy after the launch instead of row
    by row while it runs.  Same bits."""
    V, P = 64, 1024
    tree = synth.additive_tree(n_voices=V, n_partials=P, seed=0x5EED0104)
    with Renderer(hip_lib) as a, Renderer(hip_lib, options={"FR_HOST_STREAM": "0"}) as b:
        assert a.options()["FR_HOST_STREAM"]["value"] == "1" and b.options()["FR_HOST_STREAM"]["value"] == "0"
        synth.install(a, tree)
        synth.install(b, tree)
        idx = 0
        for T in (1024, 4800, 4800):
            assert V * T * 4 >= 256 << 10
            row = synth.time_ramp(idx, idx + T)
            oa = a.fill_buffer(V, idx, idx + T, [row])
            ob = b.fill_buffer(V, idx, idx + T, [row])
            assert same_bits(oa, ob), (idx, T)
            assert np.any(oa != 0)
            idx += T
