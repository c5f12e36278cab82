"""FR_LOOP_TILES on the CPU: the engine's own host code in the host-logic simulator (tests/sim_tools.py).

This covers the RULE and its plumbing -- the option's strictness and listing, "loop_tiles" in fr_plan_json only once the
option is set, which launches of every case of tests/loop_tile_cases.py carry +tile and the reason where none does -- and that
the engine passes the same windows either way: the bits equal the option off and tests/stage_reference.py's dense reference.
It does NOT cover the kernels' arithmetic: the simulator's launch_stage interprets every launch with its plain loop and ignores
StageArgs::tile (the bits are the same by design).  stage_tile_kernel and jit_stage_tile: tests/test_hip_loop_tiles.py."""
import numpy as np
import pytest

import loop_tile_cases as L
import sim_tools
import stage_reference as sr
import stage_variants as sv
from libfriendship_amd.capi import FR_ERR_INVALID_ARG, RenderError, Renderer


@pytest.fixture(scope="module")
def sim():
    return sim_tools.sim_lib()


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("FR_LOOP_TILES", "FR_RING_KEEP", "FR_STAGE_JIT"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_option_plumbing(sim, clean_env):
    with Renderer(sim) as r:
        assert "FR_LOOP_TILES" not in r.options()
    with Renderer(sim, options={"FR_LOOP_TILES": "1"}) as r:
        assert r.options()["FR_LOOP_TILES"] == {"value": "1", "source": "option"}
    clean_env.setenv("FR_LOOP_TILES", "1")
    with Renderer(sim) as r:
        assert r.options()["FR_LOOP_TILES"] == {"value": "1", "source": "env"}
    with Renderer(sim, options={"FR_LOOP_TILES": "0"}) as r:          # the option beats the environment
        assert r.options()["FR_LOOP_TILES"] == {"value": "0", "source": "option"}
    for bad in ("2", "on", "", "-1"):
        clean_env.delenv("FR_LOOP_TILES", raising=False)
        with pytest.raises(RenderError) as ei:
            Renderer(sim, options={"FR_LOOP_TILES": bad})
        assert ei.value.status == FR_ERR_INVALID_ARG
        clean_env.setenv("FR_LOOP_TILES", bad)
        with pytest.raises(RenderError) as ei:
            Renderer(sim)
        assert ei.value.status == FR_ERR_INVALID_ARG


def test_plan_json_shows_loop_tiles_only_when_set(sim, clean_env):
    g = sv.echo((1,))
    x = [np.arange(32, dtype=np.float32), np.zeros(32, np.float32)]
    plans = {}
    for name, opts in (("unset", {}), ("off", L.OFF), ("on", L.ON)):
        with Renderer(sim, options=opts) as r:
            g.install(r)
            r.fill_buffer(1, 0, 32, x)
            plans[name] = r.plan()
    assert "loop_tiles" not in plans["unset"] and all("tile" not in l["variant"] for l in plans["unset"]["stage_launches"])
    assert plans["off"]["loop_tiles"] == {"frames": 0, "max_stride": plans["on"]["loop_tiles"]["max_stride"], "reason": "FR_LOOP_TILES is off"}
    assert plans["on"]["loop_tiles"]["frames"] == 256 and plans["on"]["loop_tiles"]["reason"] == ""
    assert 1 <= plans["on"]["loop_tiles"]["max_stride"] <= 64
    # nothing else of the plan changes with the option unset or off
    drop = ("loop_tiles", "build_ms", "lower_ms", "jit_compile_ms")
    strip = lambda p: {k: v for k, v in p.items() if k not in drop}   # noqa: E731
    assert strip(plans["unset"]) == strip(plans["off"])
    assert [l["variant"] for l in plans["on"]["stage_launches"]] == ["stage_kernel/feedback+carry_only+tile", "stage_kernel/copy"] or \
        [l["variant"] for l in plans["on"]["stage_launches"]] == ["stage_kernel/feedback+carry_only+tile"], plans["on"]["stage_launches"]


def test_a_plan_without_feedback_is_never_tiled(sim, clean_env):
    g = sv.chain((300, 600, 300))     # the strided form of an effects chain: not a loop
    rng = np.random.default_rng(1)
    with Renderer(sim, options={**L.ON, "FR_STAGE_JIT": "0"}) as r:
        g.install(r)
        for idx in (0, 517):
            r.fill_buffer(g.n_out, idx, idx + 517, [rng.normal(size=517).astype(np.float32) for _ in range(2)])
        p = r.plan()
        assert not p["feedback"] and p["loop_tiles"]["frames"] == 0 and p["loop_tiles"]["reason"] == "", p["loop_tiles"]
        assert [l["variant"] for l in p["stage_launches"]] == ["stage_kernel/strided"], p["stage_launches"]


@pytest.mark.parametrize("case", L.CASES, ids=L.IDS)
def test_case_on_the_simulator(sim, clean_env, case):
    case = L.resolve(case, L.max_stride(sim))
    g = L.build(case)
    T = case["T"]
    rng = np.random.default_rng(5)
    store = sr.InputStore()
    ref = sr.DenseReference(g, case["semantics"])
    calls = [("first", 0, T), ("steady", T, T), ("one frame", 2 * T, 1), ("seek forward", case["seek"], 64)]
    with Renderer(sim, options={**L.ON, "FR_STAGE_JIT": "0"}, semantics=case["semantics"]) as on, \
            Renderer(sim, options={"FR_STAGE_JIT": "0"}, semantics=case["semantics"]) as off:
        g.install(on)
        g.install(off)
        for what, idx, n in calls:
            rows = [(rng.normal(size=n) * 3).astype(np.float32) for _ in range(case["n_in"])]
            if what == "steady":
                rows[case["hostile"]][::5] = np.resize(sv.HOSTILE, len(rows[case["hostile"]][::5]))
            store.call(idx, rows)
            got = on.fill_buffer(g.n_out, idx, idx + n, rows)
            base = off.fill_buffer(g.n_out, idx, idx + n, rows)
            forms = L.check_launches(case, on.plan(), what)
            if what == "seek forward":
                assert "replay" in forms, forms
            p_off = off.plan()
            assert "loop_tiles" not in p_off and all("tile" not in l["variant"] for l in p_off["stage_launches"])
            # (the same launches either way; with the option on the stride is the loops' own, so a plan whose later level reads a
            #  loop's ring at another delay -- rows_inside(5): stride 5, not 1 -- also changes +carry to +carry_only)
            assert [L.form_of(l["variant"]).split("+")[0] for l in on.plan()["stage_launches"]] == \
                [L.form_of(l["variant"]).split("+")[0] for l in p_off["stage_launches"]]
            msg = sr.first_diff(got, base, f"{case['key']} {what}: option on vs off")
            assert not msg, msg
            msg = sr.first_diff(got, ref(store, idx, idx + n), f"{case['key']} {what}: vs the dense reference")
            assert not msg, msg
