"""Dense FORWARD f32 reference for graphs with feedback through Delays of a signal amount (TEST INFRASTRUCTURE, FR_LOOP_DYN).

tests/stage_reference.py evaluates a loop in blocks of its smallest CONSTANT Delay; a loop closed through a Delay of a signal
amount has none.  This reference evaluates every node once per frame, frames in time order, with stage_reference.py's operation
rules.  Within a frame the nodes run in a topological order of the graph without the source edges of the Delays that close a
loop (a Delay whose source is in its own strongly connected component): such a Delay must reach at least one frame back at
every frame, and the reference fails loudly on a frame where it does not -- it never reads a value it has not computed.  Every
other Delay may reach 0 frames back: its source comes earlier in the order.

The per-frame loop is tests/cpp/loopdyn_reference.cpp (plain C++ built with g++ on first use, no fast-math, no contraction: the
40 000-frame calls of tests/loop_dyn_cases.py over 300 loops are 10^8 node evaluations); tests/test_loop_dyn_sim.py pins it to
the C++ oracle bit for bit on the first frames of every case.
"""
import ctypes
import os
import subprocess

import numpy as np

import stage_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "loopdyn_reference.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build", "libloopdyn_reference.so")
KINDS = {"Sum2": 0, "Multiply": 1, "Divide": 2, "Modulo": 3, "Minimum": 4, "Delay": 5}
NONE, CONST, INPUT, NODE = 0, 1, 2, 3
NODE_DT = np.dtype([("kind", np.int32), ("loop", np.int32), ("a_src", np.int32), ("a_arg", np.uint32), ("b_src", np.int32), ("b_arg", np.uint32)])
_lib = None


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(OUT) or os.path.getmtime(OUT) < os.path.getmtime(SRC):
            os.makedirs(os.path.dirname(OUT), exist_ok=True)
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", OUT, SRC],
                           check=True)
        _lib = ctypes.CDLL(OUT)
        _lib.loopdyn_render.restype = ctypes.c_int64
        _lib.loopdyn_render.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                        ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p]
    return _lib


class Compiled:
    """A stage_reference.Graph as the arrays the per-frame loop reads: nodes, operands and the order within a frame."""

    def __init__(self, g):
        self.handles = [h for h in g.nodes if g.nodes[h] != "F32Constant"]
        index = {h: i for i, h in enumerate(self.handles)}
        inb = {h: {} for h in g.nodes}
        self.outs = {}
        for frm, to, fs, ts in g.edges:
            (self.outs if to == 0 else inb[to])[ts] = (frm, fs)
        succ = {h: [s for s, _ in inb[h].values() if s != 0 and g.nodes[s] != "F32Constant"] for h in self.handles}
        comp_of = {}
        for ci, comp in enumerate(sr._sccs(succ, self.handles)):
            for h in comp:
                comp_of[h] = ci
        self.nodes = np.zeros(len(self.handles), NODE_DT)
        inner = {}
        for h in self.handles:
            n = self.nodes[index[h]]
            n["kind"] = KINDS[g.nodes[h]]
            src0 = inb[h].get(0, (None,))[0]
            # (the same component: a loop through this Delay's source -- a component of one node has no edge to itself otherwise)
            closes = g.nodes[h] == "Delay" and src0 in comp_of and comp_of[src0] == comp_of[h]
            n["loop"] = 1 if closes else 0
            for slot, key in ((0, "a"), (1, "b")):
                e = inb[h].get(slot)
                if e is None:
                    n[key + "_src"] = NONE
                elif e[0] == 0:
                    n[key + "_src"], n[key + "_arg"] = INPUT, e[1]
                elif g.nodes[e[0]] == "F32Constant":
                    n[key + "_src"], n[key + "_arg"] = CONST, e[1]
                else:
                    assert e[1] == 0
                    n[key + "_src"], n[key + "_arg"] = NODE, index[e[0]]
            inner[h] = [s for s in succ[h] if not (closes and s == src0 and inb[h].get(1, (None,))[0] != s)]
        order = [c[0] for c in sr._sccs(inner, self.handles)]
        assert len(order) == len(self.handles), "a loop that no Delay closes"
        self.order = np.array([index[h] for h in order], np.int32)
        self.index = index
        self.g = g


def render(g, inputs, idx, end, semantics="reference", compiled=None):
    """The graph's output rows over [idx, end): float32 [n_out, end - idx], every frame from 0 evaluated.  `inputs`: per slot, the
    values by absolute frame (stage_reference.InputStore.rows)."""
    c = compiled or Compiled(g)
    rows = [np.ascontiguousarray(r, np.float32) for r in inputs]
    ptrs = (ctypes.c_void_p * max(len(rows), 1))(*[r.ctypes.data for r in rows])
    lens = np.array([len(r) for r in rows] + [0], np.int64)
    val = np.zeros((len(c.handles), end), np.float32)
    err = _load().loopdyn_render(c.nodes.ctypes.data, len(c.handles), c.order.ctypes.data, ptrs, lens.ctypes.data, len(rows), end,
                                 1 if semantics == "sparkle" else 0, val.ctypes.data)
    assert err == 0, f"a Delay reads a value of its own frame at frame {-err - 1}: the graph has no forward evaluation"
    n_out = g.n_out
    out = np.zeros((n_out, end - idx), np.float32)
    for r in range(n_out):
        e = c.outs.get(r)
        if e is None:
            continue
        frm, fs = e
        if frm == 0:
            row = rows[fs] if fs < len(rows) else np.zeros(0, np.float32)
            seg = row[idx:end]
            out[r, :len(seg)] = seg
        elif g.nodes[frm] == "F32Constant":
            out[r] = np.uint32(fs).view(np.float32)
        else:
            out[r] = val[c.index[frm], idx:end]
    return out


class DenseForward:
    """render() call after call on one graph (compiled once)."""

    def __init__(self, g, semantics="reference"):
        self.g, self.semantics, self.c = g, semantics, Compiled(g)

    def __call__(self, store, idx, end):
        return render(self.g, store.rows, idx, end, self.semantics, self.c)


first_diff = sr.first_diff
