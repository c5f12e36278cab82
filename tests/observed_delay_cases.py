"""Delays whose amount comes from an input, bounded by the rows observed (FR_DELAY_OBSERVED): graphs, call sequences and
a driver shared by tests/test_observed_delay_sim.py (host-logic simulator) and tests/test_hip_observed_delay.py (the HIP
library).  Every call goes to the renderer under test and to the oracle, which the outputs must match bit for bit.

Graphs: V additive voices x (slot 0 = the time ramp), each y = Sum2(x, Multiply(C(0.5), Delay(x, amount))) with the
amount read from input slot 1:
  "in"      amount = In(1)
  "affine"  amount = base + depth * In(1)
  "scaled"  amount = In(1) * 48000
None of these has a bound the planner can prove, so without the mode every row stays with the pull interpreter."""
import numpy as np

from kat_replay import same_bits
from libfriendship_amd import synth
from libfriendship_amd.capi import Renderer

F = np.float32
AMOUNTS = ("in", "affine", "scaled")
BASE, DEPTH = 100.0, 300.0


def delayed_voices(n_voices, n_partials, amount="affine", seed=0x5EED0601, base=BASE, depth=DEPTH):
    """The graph above; tree["amount_nodes"] are the handles the base constant feeds (the "affine" amount's Sum2)."""
    p = synth.voice_params(n_voices, n_partials, seed, False)
    g = synth.GraphArrays()
    leaves = synth.partial_leaves(g, p["w"], p["amp"], 0).reshape(n_voices, n_partials)
    x = synth.sum_tree(g, leaves)
    amount_nodes = None
    if amount == "in":
        amt = synth.IN(1)
    elif amount == "affine":
        amt = amount_nodes = g.binop(synth.K_SUM2, synth.C(F(base)), g.binop(synth.K_MUL, synth.C(F(depth)), synth.IN(1), n_voices), n_voices)
    elif amount == "scaled":
        amt = g.binop(synth.K_MUL, synth.IN(1), synth.C(F(48000.0)), n_voices)
    else:
        raise ValueError(amount)
    wet = g.binop(synth.K_DELAY, x, amt, n_voices)
    y = g.binop(synth.K_SUM2, x, g.binop(synth.K_MUL, synth.C(F(0.5)), wet, n_voices), n_voices)
    g.edge(y, 0, 0, np.arange(n_voices, dtype=np.uint32))
    tree = g.finish(n_voices)
    tree["amount_nodes"] = amount_nodes
    return tree


def control_row(start, end, lo, hi, seed=0):
    """A control row for slot 1: a slow ramp between lo and hi with a little deterministic wobble (not only integers)."""
    n = end - start
    u = synth.uniform01(0xC0DE0000 + seed + start, n).astype(np.float32)
    ramp = np.linspace(lo, hi, n, dtype=np.float64)
    return (ramp + (u - 0.5) * 0.01 * (hi - lo)).astype(np.float32)


def edit_base(renderers, tree, old_base, new_base):
    """Moves the "affine" amount's base constant from old_base to new_base on every renderer (one edge per voice)."""
    nodes = tree["amount_nodes"]
    for r in renderers:
        for h in nodes:
            r.on_del_edge(synth.CONST_HANDLE, int(h), int(synth.bits(old_base)), 0)
            r.on_add_edge(synth.CONST_HANDLE, int(h), int(synth.bits(new_base)), 0)


class DeviceRows:
    """fr_fill_buffer_device / _device_dense inputs and output: numpy on the simulator (its 'device' memory is host memory),
    torch tensors on the GPU."""

    def __init__(self, lib):
        self.sim = lib.path.endswith("libfr_simengine.so") or "simasan" in lib.path

    def call(self, r, n_slots, start, end, rows, dense=False):
        n = end - start
        if self.sim:
            data = np.ascontiguousarray(np.stack(rows) if dense else np.concatenate(rows), dtype=np.float32)
            out = np.zeros((n_slots, n), np.float32)
            if dense:
                r.fill_buffer_device_dense(out.ctypes.data, n_slots, n, start, data.ctypes.data, len(rows), 0)
            else:
                offs = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.uint64)
                r.fill_buffer_device(out.ctypes.data, n_slots, n, start, data.ctypes.data, offs, 0)
            return out
        import torch
        host = np.stack(rows) if dense else np.concatenate(rows)
        d_in = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).cuda()
        d_out = torch.zeros((n_slots, n), dtype=torch.float32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        if dense:
            r.fill_buffer_device_dense(d_out.data_ptr(), n_slots, n, start, d_in.data_ptr(), len(rows), stream)
        else:
            offs = np.concatenate([[0], np.cumsum([len(x) for x in rows])]).astype(np.uint64)
            r.fill_buffer_device(d_out.data_ptr(), n_slots, n, start, d_in.data_ptr(), offs, stream)
        torch.cuda.synchronize()
        return d_out.cpu().numpy()


def render(r, n_slots, start, end, rows, entry="host", dev=None):
    """One call through the given entry point: host, dense, device or device_dense."""
    if entry == "host":
        return r.fill_buffer(n_slots, start, end, rows)
    if entry == "dense":
        return r.fill_buffer_dense(n_slots, start, end, np.stack(rows))
    return dev.call(r, n_slots, start, end, rows, dense=entry == "device_dense")


def rows_for(start, end, lo, hi, seed=0):
    return [synth.time_ramp(start, end), control_row(start, end, lo, hi, seed)]


class Pair:
    """The renderer under test and the oracle, given the same graph and the same calls."""

    def __init__(self, lib, oracle_lib, tree, options=None, entry="host", **kw):
        self.r = Renderer(lib, options=options, **kw)
        self.ref = Renderer(oracle_lib, **{k: v for k, v in kw.items() if k != "history_frames"})
        self.n = tree["n_outputs"]
        self.entry = entry
        self.dev = DeviceRows(lib) if entry.startswith("device") else None
        synth.install(self.r, tree)
        synth.install(self.ref, tree)

    def call(self, start, end, rows, what=""):
        got = render(self.r, self.n, start, end, rows, self.entry, self.dev)
        exp = self.ref.fill_buffer(self.n, start, end, rows)
        assert same_bits(got, exp), f"{what} [{start}, {end}) differs from the oracle at {np.argwhere(got.view(np.uint32) != exp.view(np.uint32))[:4].tolist()}"
        return self.r.plan()

    def close(self):
        self.r.close()
        self.ref.close()


# Contiguous calls whose control values widen step by step: (frames, lo, hi).  Look-backs grow past 1, 64, 512, 4096 frames
# for "in"; the other amounts scale them.
GROWTH = [(256, 0.0, 0.0), (256, 0.0, 3.0), (256, 2.0, 40.0), (320, 10.0, 500.0), (256, 400.0, 3000.0), (192, 0.0, 3000.0), (256, 5.0, 9.0)]
SCALED_GROWTH = [(256, 0.0, 0.0), (256, 0.0, 0.001), (256, 0.0, 0.01), (320, 0.0, 0.05), (256, 0.01, 0.02)]
AFFINE_GROWTH = [(256, 0.0, 0.0), (256, 0.0, 0.5), (256, 0.2, 2.0), (320, 1.0, 9.0), (256, 0.0, 1.0)]


def growth_for(amount):
    return {"in": GROWTH, "affine": AFFINE_GROWTH, "scaled": SCALED_GROWTH}[amount]


def run_growth(pair, amount, start=0, seed=0):
    """The growth sequence from `start`; returns the plans after each call."""
    plans, t = [], start
    for k, (n, lo, hi) in enumerate(growth_for(amount)):
        plans.append(pair.call(t, t + n, rows_for(t, t + n, lo, hi, seed + k), f"{amount} call {k}"))
        t += n
    return plans, t


# Special control values: each row is (label, values cycled over the call)
SPECIALS = [
    ("nan", [np.nan, 3.0, 7.5]),
    ("neg", [-5.0, -1e30, 2.0]),
    ("neg_inf", [-np.inf, 1.0]),
    ("beyond_t", [1e6, 5.0e5, 3.0]),     # >= t: reads before frame 0 (zero)
    ("pos_inf", [np.inf, 2.0]),
    ("2^64", [1.9e19, 4.0]),
]


def special_row(start, end, values):
    v = np.asarray(values, dtype=np.float32)
    return v[np.arange(start, end) % len(v)]
