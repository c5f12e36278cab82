"""Streams of different kinds one after the other on ONE renderer, on the GPU: what outlives a stream -- the control blocks, the
doorbell's form, the launch the renderer remembers (csrc/streamplan.hpp StreamLaunch) -- must not leak into the next one.  One
renderer with every FR_STREAM_* option on opens and closes a stream per graph, the graphs replaced by edits, in an order that
makes the doorbell alternate between one row and rows: plain, in, bus, general, prog, loops, plain.  After each stream's first
block fr_plan_json names the kernel that runs; every block equals, bit for bit, fr_fill_buffer of a fresh renderer with the
streaming options off, which renders after all streams are closed (stream_cases.stream_against_fill_buffer says why)."""
import numpy as np
import pytest

import stream_cases as K
import stream_loop_cases as L
import stream_sequence_cases as S
from libfriendship_amd.capi import Renderer

pytestmark = pytest.mark.gpu


def test_streams_of_alternating_doorbell_forms_on_one_renderer(hip_lib, monkeypatch):
    for k in S.OPTIONS:
        monkeypatch.delenv(k, raising=False)
    rng = np.random.default_rng(11)
    streamed = []
    with Renderer(hip_lib, options=S.OPTIONS) as r:
        graphs = S.Graphs(r)
        for kind in S.ORDER:
            kernel, build, n_rows, n_in = S.KINDS[kind]
            tree = build()
            graphs.put(tree)
            blocks = L.blocks_of(K.short_blocks(), rng, n_in)
            r.stream_begin(n_rows)
            got = []
            for k, (idx, T, rows) in enumerate(blocks):
                got.append(r.stream_block_rows(idx, rows, n_times=T))
                if k == 0:
                    s = r.plan()["stream"]
                    assert s["servable"] and s["kernel"] == kernel, (kind, s)
            r.stream_end()
            assert [a.shape for a in got] == [(n_rows, 64), (n_rows, 1), (n_rows, 37)]
            streamed.append((kind, tree, n_rows, blocks, got))
    for k, (kind, tree, n_rows, blocks, got) in enumerate(streamed):
        assert L.fill_compare(hip_lib, tree, n_rows, blocks, got, f"of stream {k} ({kind})") == 64 + 1 + 37
        assert max(np.abs(np.where(np.isfinite(a), a, 0)).max() for a in got) > 0.01
