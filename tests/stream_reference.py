"""Dense f32 reference for block streaming (TEST INFRASTRUCTURE): what a stream of blocks must return, computed by
tests/stage_reference.py's `render` -- numpy float32, every node once per frame, the reference's operation order -- and by
nothing of the engine.  Every `synth` tree is made of the seven primitives, so `render` evaluates a whole patch, voices
included.

A stream is a list of blocks [(idx, T, rows)] with one full-length row per input slot.  Its SEGMENTS are the runs of
consecutive blocks: a segment starts at the stream's first block and at every block whose idx is not the previous block's
end (csrc/engine.cpp stream_block_rows: seek = !have_last || idx != head).  At a seek the engine rebuilds every delay line
and loop from frame 0 with every input slot 0.0 -- time included -- at all frames before the block (InputStore's seek rule),
so a segment's inputs are zeros up to its first frame and the blocks' rows after it; `expected_blocks` renders each segment
once over [first, end) and cuts the blocks out of it.  The store's rules for short rows, padding and the vector count are not
restated here: tests/test_hip_stream_inputs.py has them."""
import numpy as np

import stage_reference as R
from libfriendship_amd import synth
from libfriendship_amd.capi import PRIMITIVES


def graph_of(tree):
    """The stage_reference.Graph of a synth tree: K_* kinds by their primitive names, edges as they are."""
    g = R.Graph()
    g.nodes = {int(h): PRIMITIVES[int(k)] for h, k in zip(tree["handles"], tree["kinds"])}
    g.edges = [tuple(int(x) for x in e) for e in tree["edges"]]
    return g


def segments_of(blocks):
    """[[block numbers]]: the runs of consecutive blocks of one stream."""
    segs = []
    for k, (idx, T, _) in enumerate(blocks):
        if k and idx == blocks[k - 1][0] + blocks[k - 1][1]:
            segs[-1].append(k)
        else:
            segs.append([k])
    return segs


def expected_blocks(tree, blocks, semantics="reference"):
    """[float32 [n_out, T]] per block of the stream `blocks` = [(idx, T, rows)], rows of the block's full length."""
    g = graph_of(tree)
    out = [None] * len(blocks)
    for seg in segments_of(blocks):
        first = blocks[seg[0]][0]
        end = blocks[seg[-1]][0] + blocks[seg[-1]][1]
        n_in = max(len(blocks[k][2]) for k in seg)
        inputs = []
        for s in range(n_in):
            parts = [np.zeros(first, np.float32)]
            for k in seg:
                idx, T, rows = blocks[k]
                assert len(rows) == n_in and len(rows[s]) == T, "a stream's reference takes one full-length row per slot and block"
                parts.append(np.asarray(rows[s], np.float32))
            inputs.append(np.concatenate(parts))
        full = R.render(g, inputs, first, end, semantics)
        for k in seg:
            idx, T, _ = blocks[k]
            out[k] = full[:, idx - first:idx - first + T].copy()
    return out


def _constant_delay_edges(tree):
    """The numbers of the edges that carry a constant amount into a Delay."""
    delay = set(int(h) for h in tree["handles"][tree["kinds"] == synth.K_DELAY])
    e = tree["edges"]
    return [i for i in np.nonzero((e[:, 0] == synth.CONST_HANDLE) & (e[:, 3] == 1))[0] if int(e[i, 1]) in delay]


def constant_delays(tree):
    """The amounts of the tree's Delays of a constant amount (float32)."""
    return tree["edges"][_constant_delay_edges(tree), 2].astype(np.uint32).view(np.float32)


def with_delays_raised(tree, by=1.0):
    """The tree with every constant Delay amount raised by `by` frames."""
    e = tree["edges"].copy()
    at = _constant_delay_edges(tree)
    e[at, 2] = (e[at, 2].astype(np.uint32).view(np.float32) + np.float32(by)).astype(np.float32).view(np.uint32)
    return dict(tree, edges=e)


def rows_behind_constant_delays(tree):
    """The output rows whose value depends on a Delay of a constant amount, sorted."""
    e = tree["edges"]
    sources = {}
    for frm, to, _, _ in e:
        sources.setdefault(int(to), []).append(int(frm))
    delay = set(int(e[i, 1]) for i in _constant_delay_edges(tree))
    rows = []
    for frm, to, _, ts in e:
        if to != 0:
            continue
        seen, work, hit = set(), [int(frm)], False
        while work and not hit:
            h = work.pop()
            if h in seen or h in (0, synth.CONST_HANDLE):
                continue
            seen.add(h)
            hit = h in delay
            work.extend(sources.get(h, ()))
        if hit:
            rows.append(int(ts))
    return sorted(rows)


def first_diff(got, exp, what):
    """stage_reference.first_diff: '' when equal bit for bit (NaN == NaN, +0 != -0), else the first differing row and frame
    with both bit patterns."""
    return R.first_diff(got, exp, what)


def finite_share(blocks_out, from_frame=None, idxs=None):
    """Per output row, the share of finite samples of a list of [n_out, T] blocks (`from_frame` with the blocks' `idxs`: only
    the frames at or beyond it)."""
    cols = []
    for k, a in enumerate(blocks_out):
        if from_frame is not None:
            a = a[:, max(0, from_frame - idxs[k]):]
        cols.append(a)
    a = np.concatenate(cols, axis=1)
    return np.isfinite(a).mean(axis=1) if a.shape[1] else np.ones(a.shape[0])
