// callplan.hpp -- what one render call does with a staged plan: how large the delay-line rings must be, which window of
// frames the staged part renders (just the call's, or a look-back rebuilt in front of it), whether a feedback plan replays
// from frame 0, how the exchange window of a partial-block-sharded plan is cut into time tiles, and which launch form the
// stage programs run in.  Plain host logic, no HIP runtime calls, all inline (as bankplan.hpp, streamplan.hpp): the engine
// asks it before it enqueues anything, the host-logic simulator compiles it with the engine, and the test-side simulators
// (tests/cpp/plan_tests.cpp) ask the same rule; tests/cpp/callplan_tests.cpp pins its answers.
//
// The rule changes nothing.  Between ring_capacity and call_windows the engine grows or keeps its rings (engine.cpp
// prepare_rings), which decides CallIn::rings_valid.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>

#include "stage.hpp"

namespace fr {

// Feedback plans (stage.hpp StagedPlan::feedback): no window bounds a loop's look-back, so rings that are not current are
// brought up to date by replaying every frame from 0 in chunks of FB_CHUNK frames; a call further out than FB_MAX_REPLAY
// is refused.
constexpr uint64_t FB_CHUNK = 16384, FB_MAX_REPLAY = 1ull << 28;

// Floats per ring for a call of `n_times` frames: the power of two >= 1024 that holds the deepest look-back and the call
// (a feedback plan's rings always have room for a replay chunk: growing them later would lose the loop's state).
inline uint64_t ring_capacity(const StagedPlan &sp, uint64_t n_times) {
    const uint64_t need = sp.lmax + std::max<uint64_t>(n_times, sp.feedback ? FB_CHUNK : 0);
    uint64_t cap = 1024;
    while (cap < need) cap <<= 1;
    return cap;
}

struct CallIn {
    uint64_t idx = 0, n_times = 0;
    bool rings_valid = false;        // the rings, after any growth for this call, hold the plan's frames and end at idx
    bool keep_on = false;            // FR_RING_KEEP is in force: whatever is not current is repaired up to idx before the call
    bool repair_replay = false;      // ... and that repair replays a feedback plan's loops from frame 0
};

struct CallWindows {
    uint64_t w0 = 0, w_len = 0;      // the staged part's window: [idx, idx + n_times), or with the look-back in front of it
    bool rings_current = false;      // the rings hold everything before idx that this call reads
    bool fb_replay = false;          // a feedback plan's rings are first replayed over [0, idx)
    uint64_t x0 = 0, xlen = 0;       // the window every rank renders its split voices over (partial-block sharding)
};

// Contiguous with what the rings already hold: just this call's frames.  Otherwise (first call, seek, graph edit, larger
// call): the look-back is rebuilt from the input history, [idx - lmax, idx) in front of the call; a feedback plan replays
// instead, and its own window is the call's (the replay has brought the rings to idx by the time it runs).
inline CallWindows call_windows(const StagedPlan &sp, const CallIn &c) {
    CallWindows w;
    w.w0 = c.idx;
    if (sp.uses_rings()) {
        w.rings_current = c.keep_on || c.rings_valid;
        if (!w.rings_current && !sp.feedback) w.w0 = c.idx > sp.lmax ? c.idx - sp.lmax : 0;
    }
    w.fb_replay = sp.feedback && !c.keep_on && !w.rings_current && c.idx != 0;
    if ((c.repair_replay || w.fb_replay) && c.idx > FB_MAX_REPLAY)
        throw Error(FR_ERR_UNSUPPORTED, "a feedback loop's state at frame " + std::to_string(c.idx) + " would take replaying more than 2^28 frames");
    w.w_len = c.idx + c.n_times - w.w0;
    // Split voices: every rank renders its sub-trees over the SAME window -- the look-back window when any split voice
    // feeds a ring (lmax, ring capacity and validity are the same on every rank: same graph, same calls), else just this
    // call's frames.
    bool x_ring = false;
    for (const SplitVoice &v : sp.split) x_ring = x_ring || v.to_ring;
    w.x0 = x_ring ? w.w0 : c.idx;
    w.xlen = x_ring ? w.w_len : c.n_times;
    return w;
}

// One tile, the serial exchange: asked for (FR_SHARD_SERIAL_EXCHANGE), or the host-callback transport with neither tile option
// given -- it pays a host round trip and a stream synchronisation per message (4 tiles over gloo measured 0.63 ms per call
// against 0.28 serial, profiles/r03_exchange_rehearsal.txt), where RCCL sends are enqueued like kernels and tiling hides them.
inline bool exchange_serial(bool serial_flag, bool rccl, bool tiles_explicit) { return serial_flag || (!rccl && !tiles_explicit); }

// Tiles of the exchange window: whole 64-frame kernel tiles, at most `max_tiles` of them, none shorter than `min_tile`
// (the last one takes what is left).  `serial`: one tile, the whole window.
struct ExchangeTiles {
    uint64_t xlen = 0, tile = 0;
    uint32_t count = 0;
    uint64_t offset(uint32_t i) const { return i * tile; }                         // in the window
    uint64_t frames(uint32_t i) const { return std::min(tile, xlen - i * tile); }
};
inline ExchangeTiles exchange_tiles(uint64_t xlen, bool serial, uint32_t max_tiles, uint32_t min_tile) {
    ExchangeTiles t;
    if (xlen == 0) return t;
    uint64_t nt = serial ? 1 : std::min<uint64_t>(max_tiles, xlen / std::max<uint32_t>(min_tile, 64u));
    nt = std::max<uint64_t>(nt, 1);
    t.xlen = xlen;
    t.tile = (((xlen + nt - 1) / nt) + 63) / 64 * 64;
    t.count = (uint32_t)((xlen + t.tile - 1) / t.tile);
    return t;
}

// The launch form of the call's stage programs.
//  levels:   one launch per level of the plan over [w0, w0 + w_len) -- always valid;
//  fused:    steady state.  Every delayed ring read of the fused form reaches at least fused_max_frames back, so the call is
//            cut into `sub_windows` windows of `fused_step` frames, one fused launch each, when that takes fewer launches
//            than levels;
//  strided:  ... or ONE launch whose threads stride through the sub-windows themselves, when every delayed read of a program
//            ring reaches back a multiple of fused_stride frames into a ring its own program stores (the delay chains of an
//            effects patch: 2400, 4800, 7200 ...): a thread then reads only what it stored itself.  Worth it for a handful of
//            strides (each one is a dependent round trip to memory inside the launch);
//  feedback: a feedback plan's only form: a strided launch per level of the fused programs, then the row copies.
struct StageForm {
    enum Kind { none, levels, fused, strided, feedback } kind = none;
    uint64_t fused_step = 1;         // fused: frames per launch
    uint64_t sub_windows = 0;        // fused: launches; strided: strides inside the one launch
};
// `min_stride`: the shortest fused_stride the strided form is taken for; `strided_ok`: FR_STAGE_STRIDED.
// The engine's min_stride: a launch boundary costs ~5 us at these sizes, a stride a dependent round trip to memory, so the one
// launch pays only when each stride covers a few hundred frames.
constexpr uint64_t STRIDED_MIN_STRIDE = 256;
inline StageForm stage_form(const StagedPlan &sp, const CallIn &c, const CallWindows &w, uint64_t min_stride, bool strided_ok) {
    StageForm f;
    if (sp.progs.empty() || c.n_times == 0) return f;
    if (sp.feedback) { f.kind = StageForm::feedback; return f; }
    f.kind = StageForm::levels;
    const bool steady = sp.fused_count != 0 && w.w0 == c.idx && w.rings_current;
    if (!steady) return f;
    const uint64_t strided_sub = sp.fused_stride ? (c.n_times - 1) / sp.fused_stride + 1 : 0;
    if (sp.fused_stride >= min_stride && strided_sub >= 2 && strided_sub <= 8 && strided_ok) {
        f.kind = StageForm::strided;
        f.sub_windows = strided_sub;
        return f;
    }
    const size_t n_levels = sp.level_first.empty() ? 0 : sp.level_first.size() - 1;
    f.fused_step = std::max<uint64_t>(sp.fused_max_frames, 1);
    const uint64_t n_sub = (c.n_times - 1) / f.fused_step + 1;   // (n_times > 0 here; no overflow)
    if (n_sub < n_levels) {
        f.kind = StageForm::fused;
        f.sub_windows = n_sub;
    }
    return f;
}

// A call of ZERO own frames (CallIn::n_times == 0): what a stream that continues the input store (FR_STREAM_STORE) asks for
// before its resident launch starts at idx -- the rings brought up to idx the way the first fr_fill_buffer call of the plan at
// idx would bring them, before that call's own frames.  call_windows answers it as it stands: nothing when the rings are
// current (w_len == 0, no replay); a kept plan's repair (keep_on: the repair phases, and nothing here); a feedback plan's
// replay (fb_replay; its own window is empty); else the look-back window [idx - lmax, idx), which the ring-bound banks and the
// programs render level by level -- the form below -- with nothing written to the output.
inline StageForm bring_up_form(const StagedPlan &sp, const CallIn &c, const CallWindows &w) {
    StageForm f;
    if (c.n_times != 0 || sp.progs.empty() || sp.feedback || w.rings_current || w.w_len == 0) return f;
    f.kind = StageForm::levels;
    return f;
}

// Loop tiles (FR_LOOP_TILES): the strided launches of a feedback plan -- the steady call, the replay after a seek, the replay
// of kept rings -- run one wave per program that renders the window in tiles of `frames` frames: all 64 lanes fetch the
// tile's frame-only loads into LDS, lanes < stride walk their residue's frames on LDS operands and the carry, all 64 lanes
// store the tile (kernels.hip stage_tile_kernel, stagejit.cpp jit_stage_tile).  frames = stride * floor(256 / stride): a
// multiple of the stride, so lane r always owns residue r.  A plan is tiled when the option is on, it has feedback, every
// loop reads its own rings through the carry only, 1 <= stride <= LOOP_TILE_MAX_STRIDE, and
// every fused program has no Delay of a signal amount, at most LOOP_TILE_LOADS frame-only loads (S_INPUT, S_READ_INPUT, S_READ
// of a ring it does not store) and at most LOOP_TILE_STORES stores (S_STOREs, dst_ring, out_row).  Otherwise frames = 0 and
// `reason` names the first condition that failed ("" for a plan without feedback: the option does not concern it).
// LOOP_TILE_MAX_STRIDE: the kernels take strides up to 64 (a lane per residue); the rule stops where the tiled form measured faster
// than the untiled one by more than the untiled rounds' spread in BOTH evaluators (profiles/loop_tiles.txt: compiled programs win
// at d = 1, 2, 8, 16 and lose at 32 and 64 -- a wave whose 32 lanes each walk 8 frames per tile pays the tile's three phases for
// little serial work --, the interpreter wins up to 32 and ties at 64; 17..31 were not measured).
constexpr uint32_t LOOP_TILE_FRAMES = 256, LOOP_TILE_MAX_STRIDE = 16, LOOP_TILE_LOADS = 16, LOOP_TILE_STORES = 12;
struct LoopTile {
    uint32_t frames = 0;
    std::string reason;
};
inline LoopTile loop_tile(const StagedPlan &sp, bool enabled) {
    LoopTile lt;
    if (!sp.feedback) return lt;
    if (sp.fused_sweep) { lt.reason = "a loop delays by a signal amount (a sweep plan, FR_LOOP_DYN: no stride to tile)"; return lt; }
    if (!enabled) { lt.reason = "FR_LOOP_TILES is off"; return lt; }
    if (sp.fused_stride < 1 || sp.fused_stride > LOOP_TILE_MAX_STRIDE) {
        lt.reason = "the loops' stride is " + std::to_string(sp.fused_stride) + " frames (1.." + std::to_string(LOOP_TILE_MAX_STRIDE) + " are tiled)";
        return lt;
    }
    if (!sp.fused_carry_only) { lt.reason = "a loop reads its own ring further back than one stride"; return lt; }
    for (uint32_t p = sp.fused_first; p < sp.fused_first + sp.fused_count && p < sp.progs.size(); ++p) {
        const StageProg &pg = sp.progs[p];
        uint32_t loads = 0, stores = (pg.dst_ring != 0xFFFFFFFFu ? 1u : 0u) + (pg.out_row >= 0 ? 1u : 0u);
        for (uint32_t i = 0; i < pg.n_instr && pg.first_instr + i < sp.instrs.size(); ++i) {
            const StageInstr &in = sp.instrs[pg.first_instr + i];
            if (in.op == S_READ_DYN || in.op == S_READ_INPUT_DYN || in.op == S_STEP_DYN) {
                lt.reason = "fused program " + std::to_string(p - sp.fused_first) + " delays by a signal amount";
                return lt;
            }
            loads += in.op == S_INPUT || in.op == S_READ_INPUT || (in.op == S_READ && in.imm == 0) ? 1u : 0u;
            stores += in.op == S_STORE ? 1u : 0u;
        }
        if (loads > LOOP_TILE_LOADS) {
            lt.reason = "fused program " + std::to_string(p - sp.fused_first) + " has " + std::to_string(loads) + " frame-only loads (at most " +
                        std::to_string(LOOP_TILE_LOADS) + " are tiled)";
            return lt;
        }
        if (stores > LOOP_TILE_STORES) {
            lt.reason = "fused program " + std::to_string(p - sp.fused_first) + " has " + std::to_string(stores) + " stores (at most " +
                        std::to_string(LOOP_TILE_STORES) + " are tiled)";
            return lt;
        }
    }
    lt.frames = (uint32_t)(sp.fused_stride * (LOOP_TILE_FRAMES / sp.fused_stride));
    return lt;
}

// Sweeps (FR_LOOP_DYN): the launches of a sweep plan (stage.hpp StagedPlan::fused_sweep = W: frames [b, b + W) depend only on
// frames < b) -- the steady call, the replay after a seek, the edit path: every launch of the fused programs.
//  sweep   (option 1): each fused level is ONE launch of stage_sweep_kernel, a workgroup per program that renders the window
//          `frames` = min(W, LOOP_SWEEP_MAX) frames at a time, a thread per frame, a barrier between two sweeps (a shorter
//          sweep than W is as valid: the bound only has to hold);
//  windows (option 2): the same programs through stage_kernel, unchanged, one launch of stride 0 per W frames, level by level
//          inside each window -- an evaluator that rests only on a kernel the other forms have proven, and the baseline the
//          sweep kernel is measured against.
// A plan that is no sweep plan: none, and `reason` says why ("" without feedback: the option does not concern it).
constexpr uint32_t LOOP_SWEEP_MAX = 256;
struct LoopSweep {
    enum Form { none, kernel, windows } form = none;   // (kernel: the sweep form)
    uint64_t sweep = 0;              // W
    uint32_t frames = 0;             // min(W, LOOP_SWEEP_MAX): StageArgs::sweep of the sweep form
    std::string reason;
    const char *form_name() const { return form == kernel ? "sweep" : form == windows ? "windows" : ""; }
};
inline LoopSweep loop_sweep(const StagedPlan &sp, int option) {
    LoopSweep ls;
    if (!sp.feedback) return ls;
    if (option == 0) { ls.reason = "FR_LOOP_DYN is off"; return ls; }
    if (sp.fused_sweep == 0) { ls.reason = "no loop delays by a signal amount: the strided form serves the plan"; return ls; }
    ls.sweep = sp.fused_sweep;
    ls.frames = (uint32_t)std::min<uint64_t>(sp.fused_sweep, LOOP_SWEEP_MAX);
    if (option == 2) {
        ls.form = LoopSweep::windows;
        ls.reason = "FR_LOOP_DYN=2: stage_kernel, one launch per " + std::to_string(ls.sweep) + " frames and level";
    } else {
        ls.form = LoopSweep::kernel;
        ls.reason = "every read of a loop's own ring reaches at least " + std::to_string(ls.sweep) + " frames back: sweeps of " + std::to_string(ls.frames) + " frames";
    }
    return ls;
}

}  // namespace fr
