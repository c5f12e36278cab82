"""Streams of different kinds one after the other on ONE renderer: the graphs, taken from the streaming case modules at their
smallest shapes (2 voices of 128 partials; the general kernel's own smallest schedule voices, 2 of 16), and the edit that puts
one graph in the place of another.  Shared by the simulator test of fr_plan_json's "kernel" across calls
(tests/test_stream_kernel_sim.py) and the GPU test of the sequence (tests/test_hip_stream_sequence.py)."""
import numpy as np

import stream_banks_cases as M
import stream_bus_cases as B
import stream_cases as K
import stream_general_cases as G
import stream_input_cases as I
import stream_loop_cases as L
from libfriendship_amd import synth

# every streaming option (with FR_STREAM_IDLE_MS=1500, as stream_cases.STREAM_OPTIONS)
OPTIONS = dict(K.STREAM_OPTIONS, FR_STREAM_BUS="1", FR_STREAM_INPUTS="1", FR_STREAM_BANKS="1", FR_STREAM_LOOPS="1", FR_STREAM_GENERAL="1")

# (kind, kernel, builder, output rows, input rows of a block)
KINDS = {
    "plain": ("bank_stream_kernel", lambda: synth.additive_tree(2, 128), 2, 1),
    "prog": ("bank_stream_prog_kernel", lambda: synth.effects_tree(2, 128), 2, 1),
    "bus": ("bank_stream_bus_kernel", lambda: B.mixdown_tree(2, 128, 1), 1, 1),
    "in": (I.NEW_KERNEL, lambda: I.gain_tree(2, 128), 2, 3),
    "banks": ("bank_stream_banks_kernel", lambda: M.rows_tree([(2, 128), (2, 1024)]), 4, 1),
    "loops": (L.NEW_KERNEL, lambda: K.comb_tree(2, 128, 1), 2, 1),
    "general": (G.NEW_KERNEL, lambda: synth.additive_tree(2, 16), 2, 1),
}
# the doorbell's form alternates: one row, rows, one row, ...
ORDER = ["plain", "in", "bus", "general", "prog", "loops", "plain"]


def shifted(tree, by):
    """The same graph with every handle but the fixed ones (0: inputs and outputs, 1: the constant node) moved up by `by`, and
    without the constant node, which the renderer already has."""
    h, e = tree["handles"], tree["edges"].copy()
    keep = h != synth.CONST_HANDLE
    for col in (0, 1):
        e[e[:, col] > synth.CONST_HANDLE, col] += by
    return dict(tree, handles=h[keep] + np.uint32(by), kinds=tree["kinds"][keep], edges=e)


class Graphs:
    """Puts one graph after the other into a renderer by edits: the installed graph's output edges are deleted (what is left of it
    reaches no output row and is not rendered), the next graph goes in on handles of its own."""

    def __init__(self, renderer):
        self.r, self.installed, self.next = renderer, None, 0

    def put(self, tree):
        if self.installed is not None:
            for frm, to, fs, ts in self.installed["edges"]:
                if to == 0:
                    self.r.on_del_edge(int(frm), 0, int(fs), int(ts))
        tree = shifted(tree, self.next) if self.installed is not None else tree
        synth.install(self.r, tree)
        self.installed = tree
        self.next = int(tree["handles"].max())
        return tree
