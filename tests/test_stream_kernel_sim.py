"""fr_plan_json's "kernel" of block streaming across calls on ONE renderer, on the CPU (the host-logic simulator): the field
names the launch rule's choice (csrc/streamplan.hpp stream_launch) for a servable plan whose kernel the plan alone decides --
in, banks, loops, general -- before any stream is opened; for a prog, a bus and a plain plan it names the last resident launch's
kernel, and the simulator launches nothing, so "" stays whatever was begun, refused or closed before.  The expected values are
the output of the commit before the launch rule, recorded once.  (With launches: tests/test_hip_stream_sequence.py.)"""
import numpy as np
import pytest

import sim_tools
import stream_sequence_cases as S
from libfriendship_amd import synth
from libfriendship_amd.capi import RenderError, Renderer

ORDER = ["prog", "in", "bus", "banks", "plain", "loops", "prog", "general", "bus", "plain"]
# per graph: the field after the first call, after fr_stream_begin, after the block that the simulator cannot launch, after fr_stream_end
RECORDED = [
    ("prog", ["", "", "", ""]),
    ("in", ["bank_stream_in_kernel"] * 4),
    ("bus", ["", "", "", ""]),
    ("banks", ["bank_stream_banks_kernel"] * 4),
    ("plain", ["", "", "", ""]),
    ("loops", ["bank_stream_loops_kernel"] * 4),
    ("prog", ["", "", "", ""]),
    ("general", ["bank_stream_general_kernel"] * 4),
    ("bus", ["", "", "", ""]),
    ("plain", ["", "", "", ""]),
]


def kernel_sequence(lib):
    out = []
    with Renderer(lib, options=S.OPTIONS) as r:
        graphs = S.Graphs(r)
        for kind in ORDER:
            _, build, n_rows, n_in = S.KINDS[kind]
            graphs.put(build())
            rows = [synth.time_ramp(0, 64)] + [np.ones(64, np.float32)] * (n_in - 1)
            seen = []
            r.fill_buffer(n_rows, 0, 64, rows)
            s = r.plan()["stream"]
            assert s["servable"], (kind, s)
            seen.append(s["kernel"])
            if kind == "plain":                                      # (the plain path launches at once)
                with pytest.raises(RenderError):
                    r.stream_begin(n_rows)
            else:
                r.stream_begin(n_rows)
            seen.append(r.plan()["stream"]["kernel"])
            with pytest.raises(RenderError):
                r.stream_block_rows(0, rows)
            seen.append(r.plan()["stream"]["kernel"])
            r.stream_end()
            seen.append(r.plan()["stream"]["kernel"])
            out.append((kind, seen))
    return out


def test_kernel_field_across_streams_on_one_renderer(monkeypatch):
    for k in S.OPTIONS:
        monkeypatch.delenv(k, raising=False)
    assert kernel_sequence(sim_tools.sim_lib()) == RECORDED
