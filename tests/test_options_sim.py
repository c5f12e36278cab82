"""Per-renderer options (include/friendship_render_ext.h) on the CPU: the engine's own host code in the host-logic
simulator (tests/sim_tools.py) against the oracle.  fr_options_json reports value and source, an option beats the
environment, every refused option is FR_ERR_INVALID_ARG, no options is fr_renderer_create, and two renderers of one
process that differ in planning options each plan by their own and render the oracle's bits.  The kernels' side
(bank_launches, FR_JIT_FMA, the host path) is tests/test_hip_options.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sim_tools
from kat_replay import same_bits
from libfriendship_amd import synth
from libfriendship_amd.capi import (FR_ABI_VERSION, FR_ERR_INVALID_ARG, FR_ERR_NO_DEVICE, FR_ERR_UNSUPPORTED, FR_OK, RenderError,
                                    Renderer, fr_config, fr_option)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PER_RENDERER = ["FR_JIT", "FR_STAGE_JIT", "FR_JIT_FMA", "FR_JIT_CHUNKS", "FR_JIT_CHUNK_TARGET",
                "FR_BANK_TEMPLATE", "FR_BANK_LEAF", "FR_BANK_MULTI",
                "FR_BANK_SHORT", "FR_SHORT_PAIRS", "FR_SHORT_WGS", "FR_SHORT_NW", "FR_BANK_NW", "FR_BANK_F",
                "FR_HOST_MAPPED", "FR_HOST_STREAM", "FR_HOST_SMALL_KB", "FR_HOST_DIRECT",
                "FR_STREAM_IDLE_MS", "FR_STAGE_STRIDED", "FR_STAGE_BLOCK",
                "FR_EXCHANGE_TILES", "FR_EXCHANGE_MIN_TILE",
                "FR_LOWER_THREADS", "FR_LOWER_PAR_MIN_NODES", "FR_LOWER_PAR_MIN_EDIT"]
PROCESS_WIDE = ["FR_JIT_CACHE", "FR_JIT_DUMP", "FR_HOST_TRACE", "FR_LOWER_TRACE", "FR_PLAN_TRACE", "FR_LOWER_HUGEPAGES"]

DEFAULTS = {"FR_JIT": "1", "FR_STAGE_JIT": "1", "FR_JIT_FMA": "1", "FR_JIT_CHUNKS": "1", "FR_JIT_CHUNK_TARGET": "0",
            "FR_BANK_TEMPLATE": "1", "FR_BANK_LEAF": "1", "FR_BANK_MULTI": "1", "FR_BANK_SHORT": "1", "FR_SHORT_PAIRS": "1000",
            "FR_SHORT_WGS": "0", "FR_SHORT_NW": "0", "FR_BANK_NW": "0", "FR_BANK_F": "0", "FR_HOST_MAPPED": "2", "FR_HOST_STREAM": "1",
            "FR_HOST_SMALL_KB": "96", "FR_HOST_DIRECT": "1", "FR_STREAM_IDLE_MS": "2000", "FR_STAGE_STRIDED": "1", "FR_STAGE_BLOCK": "0",
            "FR_EXCHANGE_TILES": "4", "FR_EXCHANGE_MIN_TILE": "1024", "FR_LOWER_PAR_MIN_NODES": "200000", "FR_LOWER_PAR_MIN_EDIT": "16384"}

# (name, value) pairs every one of which must be refused
INVALID = [
    ("FR_NO_SUCH_SWITCH", "1"), ("fr_bank_short", "0"), ("", "1"),
    ("FR_BANK_SHORT", ""), ("FR_BANK_SHORT", "2"), ("FR_BANK_SHORT", "yes"), ("FR_BANK_SHORT", " 0"), ("FR_BANK_SHORT", "0 "),
    ("FR_JIT", "-1"), ("FR_JIT", "force"), ("FR_JIT_FMA", "0x0"), ("FR_BANK_LEAF", "1.0"),
    ("FR_STAGE_JIT", "2"), ("FR_STAGE_JIT", "Force"),
    ("FR_EXCHANGE_TILES", "0"), ("FR_EXCHANGE_TILES", "65"), ("FR_EXCHANGE_MIN_TILE", "63"), ("FR_EXCHANGE_MIN_TILE", "1048577"),
    ("FR_STREAM_IDLE_MS", "0"), ("FR_STREAM_IDLE_MS", "60001"), ("FR_STAGE_BLOCK", "17"), ("FR_HOST_MAPPED", "4"),
    ("FR_SHORT_NW", "5"), ("FR_SHORT_NW", "32"), ("FR_BANK_NW", "16"), ("FR_BANK_F", "3"), ("FR_BANK_F", "8"),
    ("FR_LOWER_THREADS", "0"), ("FR_LOWER_THREADS", "1025"), ("FR_HOST_SMALL_KB", "1048577"),
    ("FR_SHORT_PAIRS", "99999999999999999999"), ("FR_LOWER_PAR_MIN_NODES", "-5"),
] + [(name, "1") for name in PROCESS_WIDE]


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture
def clean_env(monkeypatch):
    for name in PER_RENDERER + PROCESS_WIDE:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def raw_create(rlib, pairs, n=None, null_options=False):
    """fr_renderer_create_with_options straight through ctypes; returns (status, handle)."""
    cfg = fr_config(FR_ABI_VERSION, -1, 0, 1, 0, 0, 0)
    arr = (fr_option * max(len(pairs), 1))(*[fr_option(None if k is None else k.encode(), None if v is None else v.encode()) for k, v in pairs])
    h = ctypes.c_void_p()
    st = rlib.lib.fr_renderer_create_with_options(ctypes.byref(cfg), None if null_options else arr, len(pairs) if n is None else n, ctypes.byref(h))
    return st, h


def render_plans(r, tree, n_slots, calls):
    """Render contiguous calls (lengths) from frame 0; returns the outputs and the plan after each call."""
    outs, plans, t = [], [], 0
    for T in calls:
        outs.append(r.fill_buffer(n_slots, t, t + T, [synth.time_ramp(t, t + T)]))
        plans.append(r.plan())
        t += T
    return outs, plans


def oracle_render(oracle_lib, tree, n_slots, calls):
    with Renderer(oracle_lib) as ref:
        synth.install(ref, tree)
        return render_plans(ref, tree, n_slots, calls)[0]


def test_options_json_sources(sim, clean_env):
    with Renderer(sim) as r:
        o = r.options()
    assert sorted(o) == sorted(PER_RENDERER)
    assert all(v["source"] == "default" for v in o.values()), o
    for name, value in DEFAULTS.items():
        assert o[name]["value"] == value, name
    assert int(o["FR_LOWER_THREADS"]["value"]) >= 1

    clean_env.setenv("FR_SHORT_PAIRS", "500")
    clean_env.setenv("FR_STAGE_JIT", "force")
    clean_env.setenv("FR_EXCHANGE_TILES", "999")     # the environment keeps its lenient reading: clamped, not refused
    clean_env.setenv("FR_BANK_SHORT", "banana")      # (anything but a leading '0' is on, as always)
    clean_env.setenv("FR_JIT_DUMP", "/nonexistent")  # process-wide: never an option, never listed
    with Renderer(sim) as r:
        o = r.options()
    assert o["FR_SHORT_PAIRS"] == {"value": "500", "source": "env"}
    assert o["FR_STAGE_JIT"] == {"value": "force", "source": "env"}
    assert o["FR_EXCHANGE_TILES"] == {"value": "64", "source": "env"}
    assert o["FR_BANK_SHORT"] == {"value": "1", "source": "env"}
    assert o["FR_BANK_NW"] == {"value": "0", "source": "default"}
    assert "FR_JIT_DUMP" not in o

    # an option beats the environment; the others keep their sources
    with Renderer(sim, options={"FR_SHORT_PAIRS": "200", "FR_STAGE_JIT": "0", "FR_BANK_NW": "8"}) as r:
        o = r.options()
    assert o["FR_SHORT_PAIRS"] == {"value": "200", "source": "option"}
    assert o["FR_STAGE_JIT"] == {"value": "0", "source": "option"}
    assert o["FR_BANK_NW"] == {"value": "8", "source": "option"}
    assert o["FR_EXCHANGE_TILES"] == {"value": "64", "source": "env"}
    assert o["FR_JIT"] == {"value": "1", "source": "default"}


def test_environment_is_read_when_the_renderer_is_created(sim, clean_env):
    """A renderer keeps what it read at creation; one created after the environment changed sees the new value."""
    clean_env.setenv("FR_BANK_SHORT", "0")
    with Renderer(sim) as a:
        clean_env.setenv("FR_BANK_SHORT", "1")
        with Renderer(sim) as b:
            assert a.options()["FR_BANK_SHORT"] == {"value": "0", "source": "env"}
            assert b.options()["FR_BANK_SHORT"] == {"value": "1", "source": "env"}


@pytest.mark.parametrize("name,value", INVALID)
def test_invalid_option_is_refused(sim, clean_env, name, value):
    st, h = raw_create(sim, [(name, value)])
    assert st == FR_ERR_INVALID_ARG and not h.value, (name, value, st)
    with pytest.raises(RenderError) as ei:
        Renderer(sim, options={name: value})
    assert ei.value.status == FR_ERR_INVALID_ARG


def test_malformed_option_arrays_are_refused(sim, clean_env):
    assert raw_create(sim, [("FR_BANK_SHORT", "0"), ("FR_BANK_SHORT", "0")])[0] == FR_ERR_INVALID_ARG   # the same name twice
    assert raw_create(sim, [("FR_BANK_SHORT", "0"), ("FR_JIT", "1"), ("FR_BANK_SHORT", "1")])[0] == FR_ERR_INVALID_ARG
    assert raw_create(sim, [(None, "0")])[0] == FR_ERR_INVALID_ARG
    assert raw_create(sim, [("FR_BANK_SHORT", None)])[0] == FR_ERR_INVALID_ARG
    assert raw_create(sim, [], n=2, null_options=True)[0] == FR_ERR_INVALID_ARG   # n_options > 0 without an array
    with pytest.raises(RenderError) as ei:
        Renderer(sim, options=[("FR_JIT", "0"), ("FR_JIT", "0")])
    assert ei.value.status == FR_ERR_INVALID_ARG
    # one good, one bad: no renderer either
    assert raw_create(sim, [("FR_BANK_SHORT", "0"), ("FR_STREAM_IDLE_MS", "0")])[0] == FR_ERR_INVALID_ARG
    # every per-renderer name is accepted at once, each exactly once
    st, h = raw_create(sim, [(k, v) for k, v in DEFAULTS.items()] + [("FR_LOWER_THREADS", "3")])
    assert st == FR_OK and h.value
    sim.lib.fr_renderer_destroy(h)


def test_product_library_checks_options_before_the_device(hip_lib, clean_env):
    """The product checks its options first: a refused option is FR_ERR_INVALID_ARG on any machine; a valid one gets as far
    as the device (FR_ERR_NO_DEVICE without a gfx950, a renderer with one)."""
    assert hip_lib.has_options
    for name, value in [("FR_NO_SUCH_SWITCH", "1"), ("FR_JIT_DUMP", "/tmp"), ("FR_BANK_SHORT", "2")]:
        st, h = raw_create(hip_lib, [(name, value)])
        assert st == FR_ERR_INVALID_ARG and not h.value
    st, h = raw_create(hip_lib, [("FR_BANK_SHORT", "0")])
    assert st in (FR_OK, FR_ERR_NO_DEVICE)
    if st == FR_OK:
        hip_lib.lib.fr_renderer_destroy(h)


def test_oracle_has_no_options(oracle_lib):
    assert not oracle_lib.has_options
    with pytest.raises(RenderError) as ei:
        Renderer(oracle_lib, options={"FR_BANK_SHORT": "0"})
    assert ei.value.status == FR_ERR_UNSUPPORTED
    with Renderer(oracle_lib) as r, pytest.raises(RenderError) as ei:
        r.options()
    assert ei.value.status == FR_ERR_UNSUPPORTED


STABLE = ("lower_ms", "build_ms")   # wall-clock times: the only plan keys two identical renderers may disagree on


@pytest.mark.parametrize("case", ["additive", "effects", "mixed_calls"])
def test_no_options_is_renderer_create(sim, oracle_lib, clean_env, case):
    """create_with_options(cfg, NULL, 0) plans and renders exactly like fr_renderer_create."""
    if case == "additive":
        tree, n, calls = synth.additive_tree(n_voices=3, n_partials=64, seed=11), 3, [256, 64, 700]
    elif case == "effects":
        tree, n, calls = synth.effects_tree(3, 32, taps=3, base_delay=50.0), 3, [128, 128, 300]
    else:
        tree, n, calls = synth.chorus_tree(2, 32, depth=30.0, base=40.0), 2, [1, 2, 65, 400]
    results = []
    for opts in (None, {}):
        with Renderer(sim, options=opts) as r:
            synth.install(r, tree)
            results.append(render_plans(r, tree, n, calls))
    (outs_a, plans_a), (outs_b, plans_b) = results
    exp = oracle_render(oracle_lib, tree, n, calls)
    for pa, pb in zip(plans_a, plans_b):
        assert {k: v for k, v in pa.items() if k not in STABLE} == {k: v for k, v in pb.items() if k not in STABLE}
    for a, b, e in zip(outs_a, outs_b, exp):
        assert same_bits(a, b) and same_bits(a, e)


def general_voices(V, P):
    """V voices of P partials, P not a power of two: the schedule kernel (gbank) and, for many small ones, its
    whole-voices-per-wave form."""
    base = synth.voice_params(64, P, seed=4)
    reps = V // 64 + 1
    w = (np.tile(base["w"], (reps, 1))[:V] * (1.0 + 1e-4 * (np.arange(V) // 64))[:, None]).astype(np.float32)
    amp = np.tile(base["amp"], (reps, 1))[:V].copy()
    g = synth.GraphArrays()
    leaves = synth.partial_leaves(g, w, amp).reshape(V, P)
    g.edge(synth.sum_tree(g, leaves), 0, 0, np.arange(V, dtype=np.uint32))
    return g.finish(V)


def interleaved(sim, tree, n, calls, opts_a, opts_b):
    """Two renderers alive at once, calls alternating between them; returns (outs, plans) of each."""
    res = {"a": ([], []), "b": ([], [])}
    with Renderer(sim, options=opts_a) as a, Renderer(sim, options=opts_b) as b:
        synth.install(a, tree)
        synth.install(b, tree)
        t = 0
        for T in calls:
            for key, r in (("a", a), ("b", b)):
                res[key][0].append(r.fill_buffer(n, t, t + T, [synth.time_ramp(t, t + T)]))
                res[key][1].append(r.plan())
            t += T
    return res["a"], res["b"]


def test_two_renderers_template_banks(sim, oracle_lib, clean_env):
    """FR_BANK_TEMPLATE=0 on one renderer only.  (The simulator has no run-time compiler, so a template voice sent to the
    compiled path falls back to the template there; with FR_JIT=0 as well it is planned as stage programs instead.)"""
    tree, n, calls = synth.additive_tree(n_voices=4, n_partials=64, seed=3), 4, [300, 64, 513]
    (oa, pa), (ob, pb) = interleaved(sim, tree, n, calls, None, {"FR_BANK_TEMPLATE": "0", "FR_JIT": "0"})
    exp = oracle_render(oracle_lib, tree, n, calls)
    for i, T in enumerate(calls):
        assert len(pa[i]["banks"]) == 1 and pa[i]["stage_programs"] == 0
        assert [b["kernel"] for b in pa[i]["bank_launches"]] == ["bank_kernel"] and pa[i]["bank_launches"][0]["frames"] == T
        assert pb[i]["banks"] == [] and pb[i]["stage_programs"] == 4 and pb[i]["bank_launches"] == []
        assert same_bits(oa[i], exp[i]) and same_bits(ob[i], exp[i])


def test_two_renderers_multi_voice_kernel(sim, oracle_lib, clean_env):
    """FR_BANK_MULTI=0 on one renderer only: its many small general voices go one per workgroup, the other's whole
    voices per wave."""
    V = 1400
    tree, calls = general_voices(V, 24), [200, 300]
    (oa, pa), (ob, pb) = interleaved(sim, tree, V, calls, {}, {"FR_BANK_MULTI": "0"})
    for i in range(len(calls)):
        la, lb = pa[i]["bank_launches"], pb[i]["bank_launches"]
        assert [x["kernel"] for x in la] == ["gbank"] and la[0]["voices_per_wave"] > 0
        assert [x["kernel"] for x in lb] == ["gbank"] and lb[0]["voices_per_wave"] == 0
        assert la[0]["voices"] == V and la[0]["partials"] == 24
        assert same_bits(oa[i], ob[i])
    with Renderer(oracle_lib) as ref:
        synth.install(ref, tree)
        exp = ref.fill_buffer(V, 0, 66, [synth.time_ramp(0, 66)])
    assert same_bits(oa[0][:, :66], exp)


def test_two_renderers_stage_jit(sim, oracle_lib, clean_env):
    """FR_STAGE_JIT=force against 0 on a plan with stage programs.  The simulator compiles nothing, so both plans interpret
    their programs (tests/test_hip_options.py checks the compiled one); each renderer reports its own mode, and both
    render the oracle's bits while their calls interleave."""
    tree, n, calls = synth.effects_tree(3, 32, taps=3, base_delay=50.0), 3, [128, 64, 300]
    (oa, pa), (ob, pb) = interleaved(sim, tree, n, calls, {"FR_STAGE_JIT": "force"}, {"FR_STAGE_JIT": "0"})
    exp = oracle_render(oracle_lib, tree, n, calls)
    for i in range(len(calls)):
        assert pa[i]["stage_programs"] + pa[i]["fused_programs"] > 0 and pa[i]["stage_jit"] is False and pb[i]["stage_jit"] is False
        assert same_bits(oa[i], exp[i]) and same_bits(ob[i], exp[i])


def test_option_beats_environment_in_the_plan(sim, oracle_lib, clean_env):
    """FR_BANK_MULTI=0 from the environment, =1 from an option: the option's renderer takes the multi-voice kernel."""
    V = 1400
    tree = general_voices(V, 24)
    clean_env.setenv("FR_BANK_MULTI", "0")
    (oa, pa), (ob, pb) = interleaved(sim, tree, V, [200], None, {"FR_BANK_MULTI": "1"})
    assert pa[0]["bank_launches"][0]["voices_per_wave"] == 0
    assert pb[0]["bank_launches"][0]["voices_per_wave"] > 0
    assert same_bits(oa[0], ob[0])


@pytest.mark.parametrize("lib", ["sim", "oracle"])
def test_cpp_plugin_renderer_options(sim, oracle_lib, clean_env, lib):
    """host/friendship.hpp: PluginRenderer passes options through fr_renderer_create_with_options when the library has it,
    and says so clearly when it does not."""
    src = os.path.join(ROOT, "tests", "cpp", "options_host.cpp")
    binary = os.path.join(ROOT, "tests", "cpp", "_build", "options_host")
    deps = [src, os.path.join(ROOT, "libfriendship_amd", "host", "friendship.hpp"), os.path.join(ROOT, "include", "friendship_render_ext.h")]
    if not os.path.exists(binary) or os.path.getmtime(binary) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(binary), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-pthread", "-o", binary, src, "-ldl"], check=True)
    path = sim.path if lib == "sim" else oracle_lib.path
    p = subprocess.run([binary], env=dict(os.environ, FRIENDSHIP_RENDERER_LIB=path), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = dict(line.split(": ", 1) for line in p.stdout.strip().splitlines())
    if lib == "sim":
        assert lines["plain"].startswith("ok {") and '"FR_BANK_SHORT":{"value":"1","source":"default"}' in lines["plain"]
        assert '"FR_BANK_SHORT":{"value":"0","source":"option"}' in lines["short_off"]
        assert '"FR_STAGE_JIT":{"value":"force","source":"option"}' in lines["short_off"]
        for case in ("unknown", "process_wide", "twice"):
            assert lines[case].startswith(f"status {FR_ERR_INVALID_ARG} "), lines[case]
    else:
        assert lines["plain"] == "ok "   # (the oracle has no fr_options_json: an empty description)
        for case in ("short_off", "unknown", "process_wide", "twice"):
            assert lines[case].startswith(f"status {FR_ERR_UNSUPPORTED} ") and "fr_renderer_create_with_options" in lines[case], lines[case]
