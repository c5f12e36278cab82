// stage.hpp -- plan of the staged (materialised) evaluation: fused banks + per-cut-node register programs.
#pragma once

#include <algorithm>
#include <cstdint>
#include <functional>
#include <memory>
#include <vector>

#include "graph.hpp"
#include "kernels.hpp"
#include "match.hpp"
#include "range.hpp"

namespace fr {

// Voices rendered by one bank launch.
struct BankLaunch {
    uint32_t log2_p = 0;
    uint32_t input_slot = 0;
    bool fast_ok = true;
    bool to_ring = false;            // rows are ring indices (window with look-back) instead of output rows
    bool to_ws = false;              // rows index the exchange workspace (partial-block sharding: this rank's sub-trees)
    std::vector<uint32_t> rows;      // destination row per voice
    std::vector<float> params;       // balanced: [voices][P]{w, -4*amp}; general: [groups][8]{w, -4*amp}
    bool general = false;            // voices are arbitrary Sum2 trees evaluated by schedule (match.hpp VoiceMatch)
    std::vector<uint32_t> groups;    // general: group words of all voices, concatenated
    std::vector<uint32_t> group_off; // general: [voices + 1][2] {first item, first parameter group of 8 pairs} of each voice
    uint32_t max_leaves = 0;
    // jit == true: leaves of an arbitrary common shape, kernel specialised with hipRTC (jit.hpp); params = [voices][P][k]
    bool jit = false;
    LeafShape shape;
    std::vector<bool> varying;
    std::vector<uint32_t> literal_bits;
    std::vector<uint32_t> alias;
    uint32_t k = 0;
    bool tracks = false;             // jit leaves read per-leaf track rows of the call's dense input matrix (leafshape.hpp LEAF_TRACK)
    uint32_t max_track_slot = 0;
};

// How the job is split over `world` renderers, one per GPU (friendship_render.h fr_shard).  Output rows are owned in
// contiguous blocks; every rank plans from the same graph with the same code, so what must agree between ranks -- the
// list of split voices and its order, the look-back window -- agrees by construction.
struct ShardSpec {
    uint32_t rank = 0, world = 1;
    int mode = FR_SHARD_NONE;
};
inline void shard_row_range(uint32_t rank, uint32_t world, uint32_t n_rows, uint32_t &lo, uint32_t &hi) {
    const uint32_t q = n_rows / world, r = n_rows % world;
    lo = rank * q + std::min(rank, r);
    hi = lo + q + (rank < r ? 1u : 0u);
}
inline uint32_t shard_row_owner(uint32_t row, uint32_t world, uint32_t n_rows) {
    const uint32_t q = n_rows / world, r = n_rows % world;
    const uint32_t big = r * (q + 1);   // rows held by the ranks that own q + 1 rows
    return row < big ? row / (q + 1) : r + (q ? (row - big) / q : 0);
}

// A bank voice cut at the top log2(world) levels of its Sum2 tree (FR_SHARD_PARTIALS): row i of the exchange
// workspace.  Every rank renders its own sub-tree of it; after the exchange the owner holds the voice's value and
// stores it where the unsharded plan would have: ring `dst` (to_ring) or output row `dst`.
struct SplitVoice {
    uint32_t owner = 0;
    bool to_ring = false;
    uint32_t dst = 0;
};

struct StagedPlan {
    std::vector<BankLaunch> banks;
    std::vector<SplitVoice> split;         // exchange workspace rows, in exchange order (same on every rank)
    std::vector<StageInstr> instrs;
    std::vector<StageProg> progs;          // ordered by level
    std::vector<uint32_t> level_first;     // level l = progs[level_first[l] .. level_first[l+1])
    // fused steady-state form (optional): progs[fused_first .. fused_first + fused_count) do the work of all levels in
    // one launch; valid when the rings are current and the call is at most fused_max_frames long
    uint32_t fused_first = 0, fused_count = 0;
    uint64_t fused_max_frames = 0;
    // gcd of the delays of the fused form's reads of program rings (0: there are none).  A call longer than
    // fused_max_frames is still ONE launch when its threads stride by this many frames (callplan.hpp StageForm).
    uint64_t fused_stride = 0;
    // Feedback plans (graph.hpp OP_FBREF): the fused form is the only valid one and always runs strided; its programs are
    // ordered in levels (progs[fused_first + fused_level_first[l] .. fused_first + fused_level_first[l + 1]), one launch each),
    // and progs[post_first .. post_first + post_count) copy rings to output rows after them.  Rings are brought up to date by
    // replaying the frames from 0 (there is no look-back window that bounds a loop).
    bool feedback = false;
    uint32_t feedback_loops = 0;     // cut loops the rendered rows reach
    std::vector<uint32_t> fused_level_first;
    uint32_t post_first = 0, post_count = 0;
    bool fused_carry_only = false;   // every fused program reads the rings it stores through the carry only (kernels.hpp STAGE_CARRY)
    // Sweep plans (FR_LOOP_DYN; 0: not one): a feedback plan some program of which reads a program's ring through a Delay of a
    // signal amount.  W = the least lower bound, over the fused programs after merging, of their reads of rings they store
    // themselves (a constant read: its d; a signal read: floor(lo) of its amount's proven interval, S_READ_DYN's imm): frames
    // [b, b + W) depend only on frames < b.  Such a plan has fused_stride 0, no carry annotations and runs on the interpreter
    // (callplan.hpp loop_sweep).
    uint64_t fused_sweep = 0;
    uint32_t n_rings = 0;
    uint64_t lmax = 0;                     // deepest look-back any ring must serve
    // How far back in the INPUT history the staged part can read when it computes frame t (ring look-backs + the delays
    // of inputs on top of them: constant amounts and proven bounds); `input_lookback_unbounded`: some read has no bound
    // (an input delayed by an unbounded signal, or rows left to the pull interpreter).  fr_config.history_frames.
    uint64_t input_lookback = 0;
    bool input_lookback_unbounded = false;
    std::vector<uint32_t> input_slots;     // dense input index used by programs -> external slot
    std::vector<uint32_t> pull_rows;       // output rows left to the pull interpreter
    // Observed-amount mode (ObservedInputs): the staged Delays whose bound came from the inputs' observed ranges, with the
    // look-back planned for each (a power of two at least that bound); the input slots those amounts read; signal Delays the
    // mode had to leave unstaged (an input range holding an infinity, a divisor range holding 0, a bound over the maximum).
    struct ObservedDelay { uint32_t amount; uint64_t planned; };
    std::vector<ObservedDelay> observed;
    std::vector<uint32_t> observed_slots;
    uint64_t observed_lookback = 0;
    uint32_t observed_refused = 0;
    // Track history (FR_TRACK_HISTORY): the deepest frame before the call's first one that any read of a track slot reaches
    // (ring windows of the voices that read tracks, constant delays and proven bounds on the paths from a track), and the
    // track slots that programs, the pull interpreter and template voices read through an input table (stage.cpp check_tracks)
    uint64_t track_lookback = 0;
    std::vector<uint32_t> track_window_slots;
    bool track_unbounded = false;          // (planning only) a staged read of a track by a signal amount without a bound
    // What each ring holds (FR_RING_KEEP, engine.cpp RingTable): the lowered node whose value it is -- ids are append-only and
    // hash-consed, so within one Lowering::generation() the id names the function --, the look-back it must serve (feedback
    // plans: the deepest delay it is read with; its older frames only ever matter to a replay from 0), and for feedback plans
    // the loops its value passes through: {j, fb_target[j]} of every OP_FBREF its expression reaches, through the targets too.
    // prog_rings: the rings every program stores (dst_ring and its S_STOREs).
    std::vector<uint32_t> ring_node;
    std::vector<uint64_t> ring_lookback;
    std::vector<std::vector<uint32_t>> ring_fb;
    std::vector<std::vector<uint32_t>> prog_rings;
    bool uses_rings() const { return n_rings != 0; }
};

// W of the merged fused programs of a feedback plan planned with FR_LOOP_DYN (StagedPlan::fused_sweep; 0: no program reads a
// program's ring through a Delay of a signal amount, the plan is not a sweep plan).  `instrs[first_instr - base ...]` are a
// program's instructions, S_READ_DYN's imm the proven lower bound of its amount in frames; `bank_rings`: the rings that bank
// launches fill (complete before any program runs).  Only reads of rings the reading program stores itself count: a constant
// read with its d, a signal read with its bound -- and a bound of 0 there is refused: the read may reach what is being computed.
inline uint64_t sweep_bound(const StageInstr *instrs, size_t base, const std::vector<StageProg> &progs, const std::vector<uint32_t> &bank_rings) {
    bool any = false;
    uint64_t w = ~0ull;
    for (const StageProg &pg : progs) {
        const StageInstr *ins = instrs + (pg.first_instr - base);
        auto mine = [&](uint32_t ring) {
            if (pg.dst_ring == ring) return true;
            for (uint32_t k = 0; k < pg.n_instr; ++k)
                if (ins[k].op == S_STORE && ins[k].buf == ring) return true;
            return false;
        };
        for (uint32_t k = 0; k < pg.n_instr; ++k) {
            const StageInstr &in = ins[k];
            if (in.op == S_READ_DYN && std::find(bank_rings.begin(), bank_rings.end(), in.buf) == bank_rings.end()) any = true;
            if (in.op == S_READ && mine(in.buf)) w = std::min<uint64_t>(w, in.d_lo);
            if (in.op == S_READ_DYN && mine(in.buf)) {
                if (in.imm == 0) throw Error(FR_ERR_UNSUPPORTED, "a feedback plan reads a program's ring through a signal-dependent Delay");
                w = std::min<uint64_t>(w, in.imm);
            }
        }
    }
    if (!any) return 0;
    if (w == ~0ull || w == 0) throw Error(FR_ERR_UNSUPPORTED, "internal: a sweep plan without a bound on its loops' reads");
    return w;
}

// FR_DELAY_OBSERVED: a signal Delay amount with no proven bound is bounded from the values its inputs have actually held
// since the last seek.  `range(slot)` is that slot's hull (always holding 0.0: unfed slots, zero prefixes and frames beyond
// what was stored read 0.0); a staged Delay plans a look-back of the bound rounded up to a power of two, at most
// `max_lookback` frames.  The engine re-plans when new rows widen a hull past a planned look-back (observed_plan_holds).
struct ObservedInputs {
    std::function<Range(uint32_t slot)> range;
    uint64_t max_lookback = 1u << 20;
};

// allow_banks: recognise fused oscillator banks; allow_programs: stage everything else that qualifies.
// `reuse`: a matcher built over this same FlatGraph object with the same limits, kept by the caller across plans
// (incremental re-planning after a graph edit: unchanged voices are answered from its memo).
class BankMatcher;
// `track_from`: input slots >= it are control-rate tracks (fr_set_track_inputs): visible only to the call that supplies them,
// readable only by the leaves of shape-matched voices (anything else that reads one makes the plan FR_ERR_UNSUPPORTED).
// `track_history` (FR_TRACK_HISTORY, frames): the engine keeps that many frames of every track row, so programs, the pull
// interpreter, template voices and voices that feed delay lines may read tracks too, as far back as that.
StagedPlan plan_stages(const FlatGraph &g, bool allow_banks, bool allow_programs, uint32_t max_log2_p, bool allow_jit = false,
                       bool allow_template = true, BankMatcher *reuse = nullptr, const ShardSpec *shard = nullptr, uint32_t track_from = 0xFFFFFFFFu,
                       const ObservedInputs *observed = nullptr, uint64_t track_history = 0, bool loop_stride = false,
                       bool loop_dyn = false);
// `loop_stride` (FR_LOOP_TILES): a feedback plan's fused_stride is the gcd of the delays with which its programs read rings they
// store themselves -- its loops -- and not also of their reads of rings that earlier levels have finished.
// `loop_dyn` (FR_LOOP_DYN): a feedback plan may read a program's ring through a Delay of a signal amount -- the Delay that cuts a
// loop, or a tap of a ring its own program stores, when the amount is proven >= 1 frame and never NaN (else FR_ERR_CYCLE for a
// cutting Delay, FR_ERR_UNSUPPORTED for a tap); a later level's tap needs no proof.  Such a plan is a sweep plan (fused_sweep).

// Do the observed Delays of `sp` (planned from `g` with observed ranges) still fit their planned look-backs under the ranges
// `obs` gives now?  False: some bound grew past its plan, or has none any more.
bool observed_plan_holds(const FlatGraph &g, const StagedPlan &sp, const ObservedInputs &obs);

}  // namespace fr
