// streamplan.hpp -- which plans block streaming (fr_stream_*, FR_STREAM_PROGRAMS=1) can serve with one resident launch, and
// how their stage programs are dealt to the voices.  Plain host logic, no HIP runtime calls, all inline (as bankplan.hpp):
// fr_stream_begin and fr_plan_json's "stream" ask the same rule, and the host-logic simulator compiles it with the engine.
//
// The resident kernel (kernels.hip bank_stream_prog_kernel) renders one bank of balanced template voices per block; wave 0 of
// the workgroup that finishes voice v holds the voice's <= 64 frames, stores them to the voice's ring and interprets the
// programs assigned to v, lane = frame.  No workgroup waits for another one's result, so inside a block a program may read
//   * at a delay < 64 frames: rings of ITS OWN voice's bank only (what its own wave has just stored),
//   * at a delay >= 64 frames: any ring (an earlier block stored those frames, and that block's done tag was seen).
// With FR_STREAM_BUS=1 (StreamEnv::bus) a program that needs two or more voices of the same block -- a mix bus -- is served
// too, still without a wait: the workgroup whose `voices_done` ticket is the last of the block (the one that writes the done
// tag) knows that every voice and every voice's programs have finished, and runs the BUS PROGRAMS before it writes the tag
// (kernels.hip bank_stream_bus_kernel).  A bus program may read below 64 frames any voice's ring and any ring that an earlier
// program of the block stores.
// With FR_STREAM_INPUTS=1 (StreamEnv::inputs) a program may read, at the current frame, input slots other than 0 -- control
// rows: a gain, a gate, a fader -- up to STREAM_MAX_INPUTS distinct slots, slot 0 included.  The block then brings one row per
// slot of StreamPlan::input_slots, in that order (kernels.hip bank_stream_in_kernel; streamrows.hpp keeps the slots' books).
// With FR_STREAM_BANKS=1 (StreamEnv::banks) a plan with 2..STREAM_MAX_BANKS bank launches -- voices of several sizes, voices
// that write rows next to voices that feed programs -- is one resident launch too (kernels.hip bank_stream_banks_kernel).
// Voices are numbered GLOBALLY, banks in plan order, then voices in bank order: everything below that says "voice" means that
// number.  Each bank has its own chunk size (deal_stream_chunks).
// With FR_STREAM_LOOPS=1 (StreamEnv::loops) a feedback plan's program may also read, below 64 frames, a ring that it stores
// ITSELF -- a loop shorter than a block: a one-pole filter, a comb above 750 Hz, a 32-frame bus echo.  Such a LOOP PROGRAM has a
// stride, the gcd of those delays (stream_loop_stride), and the one wave that runs it walks the residues of the stride in its
// lanes (kernels.hip bank_stream_loops_kernel): still nobody waits for anybody.  A read below 64 frames of a ring that an
// EARLIER program of the block stores -- the level behind a loop -- is served too: the reader follows the storer's voice.
// With FR_STREAM_GENERAL=1 (StreamEnv::general) a voice may have any partial count and any Sum2 tree: a SCHEDULE BANK -- a bank
// of general voices (items plus a merge schedule, match.hpp), or a balanced bank of 32 or 64 partials, each voice a one-item
// schedule -- gets one workgroup per voice, no chunks, and that workgroup runs the voice's schedule on its 16 waves
// (kernels.hip bank_stream_general_kernel).  Everything about programs applies to such a voice as to any other.
// With FR_STREAM_DYN=1 (StreamEnv::dyn) a program may delay a VOICE by a signal amount -- a chorus, a flanger, a delay time on a
// knob: S_READ_DYN of a bank's ring, whose offset is anything in [0, d_lo], so whatever the bound it counts as a read below a
// block and binds the program to that voice (or, with FR_STREAM_BUS, makes it a bus program); and S_STEP_DYN, which touches no
// memory.  The finishing wave has just stored the voice's frames of this block and earlier blocks stored everything older, so
// every such offset is readable and still nobody waits (kernels.hip bank_stream_dyn_kernel).  A signal delay of a ring that a
// program stores (without FR_STREAM_TAPS), one inside a loop program (without FR_STREAM_SWEEP), a delayed read of an input row and
// a bound observed from input rows stay refused.
// With FR_STREAM_HISTORY=1 (StreamEnv::history) a program may read an INPUT ROW at a delay -- a pre-delay on a control row, a
// delayed gate, Delay(In(0), d) on the time row itself: S_READ_INPUT at any constant delay, 0..63 included, in per-voice, bus and
// loop programs (there it is one more frame-only load); with FR_STREAM_DYN also S_READ_INPUT_DYN, whose amount is anything in
// [0, bound] -- the bound the planner proved for the amount and left in the instruction's `buf`; one without is refused.  The stream keeps a history of its streamed rows (kernels.hpp bank_stream_hist_kernel): workgroup 0 stores a block's
// rows there before any workgroup is released to render the block, so such a read waits for nobody, reads no voice, binds its
// program to no voice and never makes it a bus program.  Its slot is streamed like an S_INPUT's (FR_STREAM_INPUTS for a slot
// other than 0).  The deepest such read (StreamPlan::input_lookback) sizes the history, at most STREAM_HIST_MAX_FRAMES.
// S_READ_INPUT_DYN inside a loop program (without FR_STREAM_SWEEP) and a bound observed from input rows stay refused.
// With FR_STREAM_EFFECTS=1 (StreamEnv::effects) a plan with NO bank launch at all -- an echo, a comb or a flanger on a row the host
// feeds in, a gain on a control row, a one-pole smoother on a knob -- is served too, with voices == 0: its programs are dealt over
// SEGMENTS, the ordered lists of programs that one workgroup runs (kernels.hpp bank_stream_fx_kernel; one wave each).  Every
// program gets a GROUP in `run` order: it follows the group of the earlier program whose ring it reads less than a block back (the
// tap behind a loop, FR_STREAM_LOOPS) or whose ring it copies to a row, else it opens a new one; one that would follow two groups
// is a bus program (FR_STREAM_BUS), which runs in the bus segment after every segment has finished.  Group g runs in segment
// g % segments, segments = min(groups, stream_max_wgs): no plan is refused for its number of rows.  A segment stands where a
// voice stood -- voice_first has segments + 2 entries -- and still nobody waits: a read below a block is of a ring the same wave
// stored, a deeper one of an earlier block's frames.  Every other check applies to these programs unchanged.
// With FR_STREAM_TAPS=1 (StreamEnv::taps) a plan WITHOUT feedback that has no fused form -- a computed value delayed by fewer than 64
// frames or by a signal amount: a two-tap FIR behind an envelope, a chorus behind the ADSR or on the mix bus -- is served in its
// LEVEL FORM: `run` is every level's programs in level order, the row copies included.  The rule that FR_STREAM_LOOPS has for the
// level behind a loop holds for every level: an S_READ below 64 frames, 0 included, of a ring that an EARLIER program of `run`
// stores binds the reader to the storer's voice (group), so the same wave stored those frames and acknowledged them before the
// reader's loads; a reader that would follow two is a bus program (FR_STREAM_BUS, else the mix-bus refusal), and so is a reader of
// a ring that an earlier bus program stores.  With FR_STREAM_DYN also S_READ_DYN of such a ring: its offset is anything in
// [0, d_lo], a read below a block whatever the bound.  Still nobody waits.  A feedback plan and a plan with a fused form are what
// they were; a storer that comes later in `run`, and an S_READ_DYN of a ring that no earlier program stores, stay refused.
// With FR_STREAM_SWEEP=1 (StreamEnv::sweep), on top of FR_STREAM_LOOPS and FR_STREAM_DYN, a feedback plan's loops may hold Delays by
// a signal amount: (a) a SWEEP PROGRAM reads a ring it stores itself through S_READ_DYN -- a sweep plan, FR_LOOP_DYN: a flanger with
// regeneration, a comb with vibrato --; its width w (stream_sweep_width) is the least number of frames any read of its own rings
// reaches back, S_READ_DYN.imm being the proven lower bound of an amount, and stands where a loop program's stride stands; (b) an
// S_READ_DYN of a ring that an EARLIER program of `run` stores is admitted as FR_STREAM_TAPS admits it in other plans; (c) a loop
// program of constant stride may hold S_READ_DYN of a bank's ring, S_STEP_DYN and, with a history, S_READ_INPUT_DYN.  The one wave
// that runs a loop program walks the block w frames at a time (kernels.hpp bank_stream_sweep_kernel): still nobody waits.
// With FR_STREAM_LEAVES=1 (StreamEnv::leaves) a bank of COMPILED VOICES -- voices whose leaves are not the hand-matched sine partial
// but share one arbitrary expression shape: a triangle partial, a partial times a control row, a sawtooth with a divisor; what
// fr_fill_buffer renders with a hipRTC-generated kernel -- is served as a LEAF BANK: its leaf becomes a register program
// (leafprog.hpp: at most LEAF_PROG_MAX_INSTRS instructions over LEAF_PROG_MAX_REGS registers) that the rendering waves interpret
// per partial (kernels.hpp bank_stream_leaf_kernel).  A leaf bank has voices of at least 128 partials and is chunked like a
// template bank; everything about programs, buses, loops, taps, history and store applies behind it as behind any bank, and next
// to another bank it needs FR_STREAM_BANKS like any second bank.  The input slots its leaf reads are streamed rows: slot 0 is the
// time row, any other needs FR_STREAM_INPUTS and counts towards STREAM_MAX_INPUTS.  Track voices, chunked compiled banks, compiled
// voices of 32 or 64 partials, a leaf over the interpreter's limits and a leaf bank in a sweep plan stay refused.  The rule sees
// the plan in force: while hipRTC is still compiling (or with FR_JIT=0) a plan has no compiled bank and is answered as ever.
// With FR_STREAM_TRACKS=1 (StreamEnv::tracks, on top of `leaves`) a bank of TRACK VOICES -- compiled voices whose leaves read
// per-partial track rows (fr_set_track_inputs, leafshape.hpp LEAF_TRACK) -- is a leaf bank like any other: a track read is one
// more operand kind of the leaf program (leafprog.hpp LEAF_TRK), at most LEAF_PROG_MAX_TRACKS distinct ones per leaf, and a block
// brings its matrix (fr_stream_block_dense) through a staging of the rows [track_from, the highest slot a bank's table names],
// at most STREAM_MAX_TRACK_ROWS of them.  A track history, a program that reads a track (the planner's check_tracks), and what
// stays refused for every leaf bank stay refused.
// HOW a served plan is launched is one rule as well (stream_path, stream_launch, plain_stream_launch, at the end): the path, the
// kernel, its doorbell form, its tables, the loop limits, the workgroups.  fr_stream_begin, the seek, the block, the stop and
// fr_plan_json's "kernel" read the StreamLaunch it returns and decide nothing themselves.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "leafprog.hpp"
#include "stage.hpp"

namespace fr {

constexpr uint32_t STREAM_BLOCK = 64;        // the longest block a stream accepts
constexpr uint32_t STREAM_MAX_WGS = 256;     // (= kernels.hpp BANK_STREAM_WGS)
constexpr uint32_t STREAM_MAX_INPUTS = 8;    // most distinct input slots the streamed programs may read, slot 0 included (= kernels.hpp BANK_STREAM_ROWS)
constexpr uint32_t STREAM_MAX_BANKS = 8;     // most bank launches one resident launch serves (= kernels.hpp BANK_STREAM_BANKS)
// A loop program's S_INPUTs and S_READs are numbered into the kernel's load tile, the rings it stores into its store tile
// (= kernels.hpp BANK_STREAM_LOOP_LOADS / _STORES: 256 bytes of LDS per slot, 12 KiB in all next to the interpreter's 12 KiB of
// registers and the 8 KiB copy of the program's instructions: 36 880 bytes for the kernel -- one workgroup per CU is
// resident and may declare 160 KiB, so LDS is not what limits anything; the numbers are twice and 4/3 of the loop-tile
// rule's 16 and 12, and powers of two because the kernel masks its slots)
constexpr uint32_t STREAM_LOOP_LOADS = 32, STREAM_LOOP_STORES = 16;
// A schedule voice is rendered by ONE workgroup, and a block is only as fast as its slowest workgroup: the limit is four times
// the largest chunk a workgroup of a chunked bank renders (8192 partials), 16 waves x one full item of 2048 leaves.  Dealing the
// items of one voice over several workgroups is not built.
constexpr uint32_t STREAM_GENERAL_MAX_LEAVES = 32768;
constexpr uint32_t STREAM_SCHEDULE_MAX_DEPTH = 16;   // (= kernels.hip GB_MAX_DEPTH: the evaluation stack's columns in LDS)
// The deepest delayed read of an input row a stream serves (FR_STREAM_HISTORY): the history holds the next power of two above
// look-back + a block per streamed row -- at this limit 4 MiB per row, 32 MiB for STREAM_MAX_INPUTS rows.
constexpr uint64_t STREAM_HIST_MAX_FRAMES = 1ull << 20;
// The most track rows a stream stages per block (FR_STREAM_TRACKS): 256 workgroups x 128 partials x 2 rows, the largest one-chunk
// patch a whole device holds; [rows][64] floats of mapped pinned memory, 16 MiB at the limit.
constexpr uint32_t STREAM_MAX_TRACK_ROWS = 65536;
static_assert(STREAM_MAX_TRACK_ROWS == BANK_STREAM_TRACK_ROWS && LEAF_PROG_MAX_TRACKS == BANK_STREAM_LEAF_TRACKS, "the staging's limits are the kernel's");
static_assert(LEAF_PROG_MAX_INSTRS == BANK_STREAM_LEAF_INSTRS && LEAF_PROG_MAX_REGS == BANK_STREAM_LEAF_REGS && LEAF_OP_SUM2 == OP_SUM2 && LEAF_OP_MIN == OP_MIN,
              "the leaf program's limits and ops are the kernel's");
static_assert(STREAM_LOOP_LOADS == BANK_STREAM_LOOP_LOADS && STREAM_LOOP_STORES == BANK_STREAM_LOOP_STORES && STREAM_BLOCK == BANK_STREAM_LOOP_MAX_STRIDE + 1,
              "the rule's limits are the kernel's");

// What the rule needs to know besides the plan.
struct StreamEnv {
    uint32_t n_slots = 0;
    uint32_t device_cus = 0;         // 0: unknown (the simulator): the kernel's own limit stands in
    uint32_t leaf_variant = 1;       // FR_BANK_LEAF
    bool pull_mode = false;          // FR_MODE_PULL
    bool sharded = false;
    bool track_history = false;      // FR_TRACK_HISTORY is on (every call appends to the track rings)
    bool bus = false;                // FR_STREAM_BUS: programs that read several voices of a block run after the last voice
    bool inputs = false;             // FR_STREAM_INPUTS: programs may read input slots other than 0 at the current frame
    bool banks = false;              // FR_STREAM_BANKS: 2..STREAM_MAX_BANKS bank launches in one resident launch
    bool loops = false;              // FR_STREAM_LOOPS: feedback loops shorter than a block, and the taps behind them
    bool general = false;            // FR_STREAM_GENERAL: schedule banks -- general voices, balanced voices of 32 or 64 partials
    bool dyn = false;                // FR_STREAM_DYN: Delays of a voice by a signal amount (S_READ_DYN of a bank's ring, S_STEP_DYN)
    bool history = false;            // FR_STREAM_HISTORY: delayed reads of input rows (S_READ_INPUT; with `dyn` S_READ_INPUT_DYN) from the stream's history
    bool effects = false;            // FR_STREAM_EFFECTS: plans without a bank launch: the programs are dealt over segments (StreamPlan::segments)
    bool taps = false;               // FR_STREAM_TAPS: the level form of a plan without feedback; short and signal delays of a ring an earlier program stores
    bool programs = false;           // FR_STREAM_PROGRAMS: the program path exists (stream_path; plan_stream does not ask)
    bool sweep = false;              // FR_STREAM_SWEEP: Delays by a signal amount inside feedback loops shorter than a block (with `loops` and `dyn`)
    bool leaves = false;             // FR_STREAM_LEAVES (with `programs`): compiled voices as leaf banks, their leaves interpreted (leafprog.hpp)
    bool tracks = false;             // FR_STREAM_TRACKS (with `leaves` and `programs`): track voices as leaf banks, the block's matrix staged
    uint32_t track_from = 0xFFFFFFFFu;   // ... and the first declared track slot (fr_set_track_inputs; none: 0xFFFFFFFF)
    bool store = false;              // FR_STREAM_STORE, and not inert (streamstore.hpp): the launch stores the streamed rows; every plan takes the program path
};

// One bank of a streamed plan.  Voices [first_voice, first_voice + voices) of the global numbering; workgroups
// [first_wg, first_wg + (voices << (log2_p - chunk_log2))) of the launch, voice-major, then chunk.
struct StreamBank {
    uint32_t first_voice = 0, voices = 0, log2_p = 0, chunk_log2 = 0;
    bool to_ring = false;
    uint32_t first_wg = 0;
    bool general = false;            // a schedule bank (StreamEnv::general): one workgroup per voice, log2_p == chunk_log2
    uint32_t max_leaves = 0;         // ... and its largest voice
    bool leaf = false;               // a leaf bank (StreamEnv::leaves): compiled voices, chunked like a template bank
};

// Every workgroup of the launch must be resident at once, one per CU: as many as the device has CUs (0: unknown, the kernel's
// own limit stands in), and no more than the kernel's limit.
inline uint64_t stream_max_wgs(uint32_t device_cus) { return std::min<uint64_t>(STREAM_MAX_WGS, device_cus ? device_cus : STREAM_MAX_WGS); }

// The chunk size of every bank (voices, log2_p set; chunk_log2 and first_wg are written).  Every bank starts at one chunk per
// voice; false when even that is more than max_wgs workgroups.  Then, until no bank qualifies: the bank with the largest chunk
// (on a tie the lower index) among those whose chunk is above 128 partials (a wave needs a group of 8), that have fewer than
// 256 chunks per voice and whose halving keeps the total within max_wgs, has its chunk halved.  A block is only as fast as its
// largest chunk, so this evens out the partials per workgroup; for one bank it is the short-call kernel's loop.
// A schedule bank (StreamBank::general) counts as `voices` workgroups and is never halved.
inline bool deal_stream_chunks(std::vector<StreamBank> &banks, uint64_t max_wgs) {
    uint64_t total = 0;
    for (StreamBank &b : banks) { b.chunk_log2 = b.log2_p; total += b.voices; }
    if (total > max_wgs) return false;
    for (;;) {
        StreamBank *pick = nullptr;
        for (StreamBank &b : banks) {
            if (b.general || !(b.chunk_log2 > 7 && b.log2_p - b.chunk_log2 < 8)) continue;
            if (total + ((uint64_t)b.voices << (b.log2_p - b.chunk_log2)) > max_wgs) continue;
            if (!pick || b.chunk_log2 > pick->chunk_log2) pick = &b;
        }
        if (!pick) break;
        total += (uint64_t)pick->voices << (pick->log2_p - pick->chunk_log2);
        --pick->chunk_log2;
    }
    uint32_t wg = 0, v = 0;
    for (StreamBank &b : banks) {
        b.first_wg = wg;
        b.first_voice = v;
        wg += b.voices << (b.log2_p - b.chunk_log2);
        v += b.voices;
    }
    return true;
}

// The schedule of voice `voice` of a bank in the general form (kernels.hpp BankArgs::groups / group_off): at least one item,
// every item of at most 2^11 leaves, an evaluation stack that never underflows, never holds more than
// STREAM_SCHEDULE_MAX_DEPTH values and ends with exactly one.  Host only: every voice is checked before anything is uploaded.
inline bool stream_schedule_ok(const std::vector<uint32_t> &groups, const std::vector<uint32_t> &group_off, uint32_t voice, std::string *why = nullptr) {
    auto bad = [&](const std::string &w) { if (why) *why = w; return false; };
    if ((size_t)2 * voice + 2 >= group_off.size()) return bad("a voice without a schedule");
    const uint32_t i0 = group_off[2 * voice], i1 = group_off[2 * voice + 2];
    if (i0 >= i1 || i1 > groups.size()) return bad("an empty schedule");
    uint32_t depth = 0;
    for (uint32_t i = i0; i < i1; ++i) {
        const uint32_t k = groups[i] & 15u, merges = groups[i] >> 4;
        if (k > 11u) return bad("an item of more than 2048 leaves");
        if (merges > depth) return bad("the schedule's stack underflows");
        depth -= merges;                  // v = pop() + v, `merges` times; then push(v)
        if (++depth > STREAM_SCHEDULE_MAX_DEPTH) return bad("the schedule's stack is deeper than " + std::to_string(STREAM_SCHEDULE_MAX_DEPTH));
    }
    if (depth != 1) return bad("the schedule leaves " + std::to_string(depth) + " values");
    return true;
}

// The leaves of that voice (padding pairs are not leaves).
inline uint64_t stream_schedule_leaves(const std::vector<uint32_t> &groups, const std::vector<uint32_t> &group_off, uint32_t voice) {
    uint64_t n = 0;
    for (uint32_t i = group_off[2 * voice]; i < group_off[2 * voice + 2] && i < groups.size(); ++i) n += 1ull << (groups[i] & 15u);
    return n;
}

// The parameter pairs that voice's items hold, from its first group on (an item of fewer than 8 leaves is padded to 8 pairs).
inline uint64_t stream_schedule_pairs(const std::vector<uint32_t> &groups, const std::vector<uint32_t> &group_off, uint32_t voice) {
    uint64_t n = 0;
    for (uint32_t i = group_off[2 * voice]; i < group_off[2 * voice + 2] && i < groups.size(); ++i) n += std::max<uint64_t>(8, 1ull << (groups[i] & 15u));
    return n;
}

// The one-item schedules of a balanced bank of `voices` voices of 1 << log2_p partials (log2_p <= 11), in the general form: voice
// v is the item log2_p | 0 << 4, its parameters start at group v << (log2_p - 3) -- where the balanced layout has them.
inline void stream_balanced_schedule(uint32_t voices, uint32_t log2_p, std::vector<uint32_t> &groups, std::vector<uint32_t> &group_off) {
    groups.assign(voices, log2_p);
    group_off.clear();
    for (uint32_t v = 0; v <= voices; ++v) {
        group_off.push_back(v);
        group_off.push_back(v << (log2_p - 3u));
    }
}

struct StreamPlan {
    bool servable = false;
    std::string reason;              // why not ("" when servable)
    uint32_t voices = 0, chunk_log2 = 0, chunks = 0;   // chunks per voice; one bank: the launch has voices * chunks workgroups
    bool store = false;                  // the launch appends the streamed rows to the input store (StreamEnv::store): the store forms
    uint32_t segments = 0;               // a plan without a voice (StreamEnv::effects): the workgroups its programs are dealt over; 0 for every plan with voices
    bool bank_to_ring = false;
    std::vector<StreamBank> banks;       // one per bank launch, in plan order.  Several: `voices` is their total, `chunks` the
                                         // largest per-voice chunk count, chunk_log2 / bank_to_ring are bank 0's
    uint32_t workgroups() const {
        uint32_t n = 0;
        for (const StreamBank &b : banks) n += b.voices << (b.log2_p - b.chunk_log2);
        return n;
    }
    std::vector<uint32_t> progs;         // indices into StagedPlan::progs, voice by voice, then the bus programs, in the order they run
    std::vector<uint32_t> loop_stride;   // per entry of `progs`: the stride of a loop program (1..63), 0 for any other (StreamEnv::loops)
    bool has_loops() const { return std::any_of(loop_stride.begin(), loop_stride.end(), [](uint32_t l) { return l != 0; }); }
    std::vector<uint32_t> sweep_width;   // per entry of `progs`: the width of a sweep program (1..63, = its loop_stride), 0 for any other (StreamEnv::sweep)
    bool sweep_loops = false;            // a loop program of constant stride holds a Delay by a signal amount: it needs the sweep walk too
    bool has_sweep() const { return sweep_loops || std::any_of(sweep_width.begin(), sweep_width.end(), [](uint32_t w) { return w != 0; }); }
    std::vector<uint32_t> voice_first;   // [voices + 2] into `progs`: [voice_first[voices], voice_first[voices + 1]) is the bus segment
                                         // (a plan without a voice: [segments + 2], a segment where a voice stands)
    uint64_t min_ring_delay = 0;         // shortest delayed read of a ring that a program stores (0: there is none)
    uint64_t lookback = 0;               // deepest ring read of the assigned programs
    uint32_t dyn_reads = 0;              // the assigned programs' S_READ_DYNs (StreamEnv::dyn) ...
    uint32_t dyn_steps = 0;              // ... and their S_STEP_DYNs
    bool has_dyn() const { return dyn_reads + dyn_steps != 0; }
    uint32_t levels = 1;                 // the levels of the run form (StreamEnv::taps); 1 for a fused or one-level plan
    uint32_t short_reads = 0;            // ALL the assigned programs' reads below a block of rings that programs store -- a loop program's own-ring
                                         // reads, the tap behind a loop and a feedback plan's row copies as well as what StreamEnv::taps admits --, ...
    uint32_t dyn_ring_reads = 0;         // ... of which S_READ_DYNs (counted in dyn_reads too)
    uint32_t hist_reads = 0;             // the assigned programs' S_READ_INPUTs (StreamEnv::history) ...
    uint32_t hist_dyn_reads = 0;         // ... and their S_READ_INPUT_DYNs
    uint64_t input_lookback = 0;         // the deepest input read of the assigned programs: S_READ_INPUT's d_lo, S_READ_INPUT_DYN's proven bound (its buf)
    bool has_hist() const { return hist_reads + hist_dyn_reads != 0; }
    std::vector<uint32_t> input_slots{0};   // the distinct input slots the voices and the assigned programs read: slot 0 (the voices' time)
                                         // first, the others ascending -- the order of a block's streamed rows
    std::vector<uint32_t> general_voices;   // the leaf count of every voice served by schedule, in global voice order (StreamEnv::general)
    bool has_general() const { return std::any_of(banks.begin(), banks.end(), [](const StreamBank &b) { return b.general; }); }
    std::vector<LeafProgram> leaf_progs;    // per bank, in plan order: a leaf bank's program (StreamEnv::leaves); any other bank's is empty (k == 0)
    bool has_leaves() const { return std::any_of(banks.begin(), banks.end(), [](const StreamBank &b) { return b.leaf; }); }
    // FR_STREAM_TRACKS: the staged rows are the slots [track_first, track_first + track_rows) (0 rows: no leaf bank reads a track)
    uint32_t track_first = 0, track_rows = 0;
    bool has_tracks() const { return track_rows != 0; }
    std::vector<uint32_t> programs_per_voice() const {
        std::vector<uint32_t> n;
        for (size_t v = 0; v + 2 < voice_first.size(); ++v) n.push_back(voice_first[v + 1] - voice_first[v]);
        return n;
    }
    uint32_t bus_programs() const { return voice_first.size() >= 2 ? voice_first[voice_first.size() - 1] - voice_first[voice_first.size() - 2] : 0; }
};

inline const char *stage_op_name(uint8_t op) {
    static const char *const names[] = {"S_CONST", "S_INPUT", "S_READ", "S_READ_INPUT", "S_STEP", "S_SUM2", "S_MUL", "S_DIV", "S_MOD", "S_MIN",
                                        "S_STORE", "S_READ_DYN", "S_READ_INPUT_DYN", "S_STEP_DYN"};
    return op < sizeof names / sizeof names[0] ? names[op] : "an unknown op";
}

// The rings a program stores: its S_STOREs' in program order, then its dst_ring; each once.  A ring's position is its STORE SLOT.
inline std::vector<uint32_t> stream_stored_rings(const StageProg &pg, const StageInstr *ins) {
    std::vector<uint32_t> rings;
    auto add = [&](uint32_t ring) { if (std::find(rings.begin(), rings.end(), ring) == rings.end()) rings.push_back(ring); };
    for (uint32_t i = 0; i < pg.n_instr; ++i)
        if (ins[i].op == S_STORE) add(ins[i].buf);
    if (pg.dst_ring != 0xFFFFFFFFu) add(pg.dst_ring);
    return rings;
}

// A program's stride: the gcd of the delays, below a block, with which it reads rings it stores itself (0: it has no such
// read, it is no loop program).  Own-ring reads of a block or more bind no lane: an earlier block stored those frames.
inline uint32_t stream_loop_stride(const StageProg &pg, const StageInstr *ins) {
    const std::vector<uint32_t> mine = stream_stored_rings(pg, ins);
    uint32_t stride = 0;
    for (uint32_t i = 0; i < pg.n_instr; ++i) {
        const StageInstr &in = ins[i];
        if (in.op != S_READ || in.d_lo == 0 || in.d_lo >= STREAM_BLOCK || std::find(mine.begin(), mine.end(), in.buf) == mine.end()) continue;
        uint32_t a = stride, b = in.d_lo;
        while (b) { const uint32_t r = a % b; a = b; b = r; }
        stride = a;
    }
    return stride;
}

// A loop program's loads as the kernel numbers them into its load tile: every S_INPUT, S_READ and S_READ_INPUT (a frame-only
// load as callplan.hpp's loop-tile rule counts it; the rule admits one with StreamEnv::history alone), in program order.
inline uint32_t stream_loop_loads(const StageProg &pg, const StageInstr *ins) {
    uint32_t n = 0;
    for (uint32_t i = 0; i < pg.n_instr; ++i) n += ins[i].op == S_INPUT || ins[i].op == S_READ || ins[i].op == S_READ_INPUT ? 1u : 0u;
    return n;
}

// The history's frames per streamed row for that look-back: the power of two >= look-back + a block.
inline uint64_t stream_hist_cap(uint64_t input_lookback) {
    uint64_t cap = STREAM_BLOCK;
    while (cap < input_lookback + STREAM_BLOCK) cap <<= 1;
    return cap;
}

// The stream's own copy of a loop program (`ins`: its pg.n_instr instructions, copied; `pg`: its streamed StageProg).  Every
// ring the program stores gets a store slot, S_STORE.imm = slot + 1; every read of one of them is marked with it, S_READ.imm =
// slot + 1, every other S_READ gets imm = 0 -- the plan's carry annotations (kernels.hpp STAGE_CARRY), which depend on
// FR_LOOP_TILES, are overwritten here and only here --; a dst_ring becomes an S_STORE of the result at the end; the stride goes
// to pg.pad[0].  False (nothing the kernel may run) when the program is no loop program or exceeds the tiles.
inline bool stream_loop_prepare(StageProg &pg, std::vector<StageInstr> &ins) {
    if (ins.size() != pg.n_instr) return false;
    const uint32_t stride = stream_loop_stride(pg, ins.data());
    const std::vector<uint32_t> mine = stream_stored_rings(pg, ins.data());
    if (stride == 0 || mine.size() > STREAM_LOOP_STORES || stream_loop_loads(pg, ins.data()) > STREAM_LOOP_LOADS) return false;
    auto slot = [&](uint32_t ring) { return (uint32_t)(std::find(mine.begin(), mine.end(), ring) - mine.begin()); };
    for (StageInstr &in : ins) {
        if (in.op == S_STORE) in.imm = slot(in.buf) + 1u;
        if (in.op == S_READ) in.imm = slot(in.buf) < mine.size() ? slot(in.buf) + 1u : 0u;
    }
    if (pg.dst_ring != 0xFFFFFFFFu) {
        StageInstr st{};
        st.op = S_STORE; st.a = (uint8_t)pg.result_reg; st.buf = pg.dst_ring; st.imm = slot(pg.dst_ring) + 1u;
        ins.push_back(st);
        pg.dst_ring = 0xFFFFFFFFu;
        ++pg.n_instr;
    }
    pg.pad[0] = stride;
    return true;
}

// A program's sweep width (FR_STREAM_SWEEP): the least number of frames that a read of a ring the program stores itself reaches
// back -- an S_READ of 1 <= d_lo < 64 counts with d_lo, an own-ring S_READ_DYN with its imm, the proven lower bound of its amount
// in frames (a sweep plan's, kernels.hpp S_READ_DYN).  0: the program has no own-ring S_READ_DYN, it is no sweep program; 64: it
// has, and no read of its own rings reaches into a block -- it runs lane = frame.  (A bound of 0 answers 0 too: the rule refuses
// it before it asks.)
inline uint32_t stream_sweep_width(const StageProg &pg, const StageInstr *ins) {
    const std::vector<uint32_t> mine = stream_stored_rings(pg, ins);
    bool any = false;
    uint32_t w = STREAM_BLOCK;
    for (uint32_t i = 0; i < pg.n_instr; ++i) {
        const StageInstr &in = ins[i];
        if ((in.op != S_READ && in.op != S_READ_DYN) || std::find(mine.begin(), mine.end(), in.buf) == mine.end()) continue;
        if (in.op == S_READ_DYN) {
            any = true;
            w = std::min(w, in.imm);
        } else if (in.d_lo >= 1 && in.d_lo < STREAM_BLOCK) {
            w = std::min(w, in.d_lo);
        }
    }
    return any ? w : 0;
}

// The stream's own copy of a sweep program: stream_loop_prepare's slot marking -- S_STORE.imm = slot + 1, S_READ.imm = slot + 1 of
// an own ring and 0 of any other, a dst_ring turned into an S_STORE --, and S_READ_DYN.imm = slot + 1 of an own ring and 0 of any
// other (the bound has been consumed: it is the width); the width goes to pg.pad[0].  False (nothing the kernel may run) when the
// program is no sweep program -- width 0 or 64 --, an own-ring S_READ_DYN has the bound 0, or the program exceeds the tiles.
inline bool stream_sweep_prepare(StageProg &pg, std::vector<StageInstr> &ins) {
    if (ins.size() != pg.n_instr) return false;
    const uint32_t w = stream_sweep_width(pg, ins.data());
    const std::vector<uint32_t> mine = stream_stored_rings(pg, ins.data());
    if (w == 0 || w >= STREAM_BLOCK || mine.size() > STREAM_LOOP_STORES || stream_loop_loads(pg, ins.data()) > STREAM_LOOP_LOADS) return false;
    auto slot = [&](uint32_t ring) { return (uint32_t)(std::find(mine.begin(), mine.end(), ring) - mine.begin()); };
    for (StageInstr &in : ins) {
        if (in.op == S_STORE) in.imm = slot(in.buf) + 1u;
        if (in.op == S_READ || in.op == S_READ_DYN) in.imm = slot(in.buf) < mine.size() ? slot(in.buf) + 1u : 0u;
    }
    if (pg.dst_ring != 0xFFFFFFFFu) {
        StageInstr st{};
        st.op = S_STORE; st.a = (uint8_t)pg.result_reg; st.buf = pg.dst_ring; st.imm = slot(pg.dst_ring) + 1u;
        ins.push_back(st);
        pg.dst_ring = 0xFFFFFFFFu;
        ++pg.n_instr;
    }
    pg.pad[0] = w;
    return true;
}

// `banks`: the plan's bank launches (the engine moves them out of StagedPlan::banks when it uploads them).
inline StreamPlan plan_stream(const StagedPlan &sp, const std::vector<const BankLaunch *> &banks, const StreamEnv &env) {
    StreamPlan s;
    s.store = env.store;
    auto refuse = [&](const std::string &why) {
        s.servable = false;
        s.reason = why;
        if (!s.voices) { s.banks.clear(); s.general_voices.clear(); s.leaf_progs.clear(); s.track_rows = 0; }   // (refused before the banks were dealt)
        return s;
    };
    if (env.n_slots == 0) return refuse("no output slots");
    if (env.sharded || !sp.split.empty()) return refuse("block streaming of a sharded renderer");
    if (env.pull_mode) return refuse("block streaming of a renderer in FR_MODE_PULL");
    if (!sp.pull_rows.empty()) return refuse(std::to_string(sp.pull_rows.size()) + " output rows are left to the pull interpreter");
    if (env.track_history || !sp.track_window_slots.empty() || sp.track_lookback != 0) return refuse("block streaming with a track history");
    // (FR_LOOP_DYN: a sweep plan's launch forms are fr_fill_buffer's alone; the resident kernels have neither -- but for the sweep
    // forms, FR_STREAM_SWEEP on top of FR_STREAM_LOOPS and FR_STREAM_DYN)
    const bool sweep = env.sweep && env.loops && env.dyn;
    if (sp.fused_sweep && !sweep) return refuse("a feedback loop delays by a signal amount (a sweep plan, FR_LOOP_DYN): block streaming does not serve it");
    const bool voiceless = env.effects && banks.empty();   // FR_STREAM_EFFECTS: the programs are dealt over segments, not voices
    if (banks.size() != 1 && !(env.banks && banks.size() >= 2 && banks.size() <= STREAM_MAX_BANKS) && !voiceless) {
        if (env.banks && banks.size() > STREAM_MAX_BANKS)
            return refuse("block streaming serves at most " + std::to_string(STREAM_MAX_BANKS) + " voice banks in one launch (this plan: " +
                          std::to_string(banks.size()) + " bank launches)");
        return refuse("block streaming needs a plan with one voice bank (this one: " + std::to_string(banks.size()) + " bank launches)");
    }
    const bool leaves = env.leaves && env.programs;  // FR_STREAM_LEAVES does nothing without FR_STREAM_PROGRAMS
    std::vector<uint32_t> others;                    // slots other than 0 that the leaves and the assigned programs read (StreamEnv::inputs)
    for (const BankLaunch *bp : banks) {             // (one bank: the checks and their order are what they have always been)
        const BankLaunch &b = *bp;
        if (leaves && b.jit) {                       // a leaf bank: compiled voices, their leaf interpreted
            const bool tracks = env.tracks && b.tracks;  // FR_STREAM_TRACKS: ... track voices too
            if (b.tracks && !tracks) return refuse("these compiled voices read per-leaf track rows (track voices); block streaming interprets leaves over constants and streamed input rows only");
            if (b.to_ws) return refuse("a compiled bank that is cut into chunks over an exchange workspace; block streaming serves whole compiled voices only");
            if (env.leaf_variant != 1) return refuse("block streaming with FR_BANK_LEAF=0");
            if (b.log2_p < 7)
                return refuse("compiled voices of " + std::to_string(1u << b.log2_p) + " partials; block streaming interprets the leaves of voices of at least 128 partials (16 waves x one group of 8)");
            if (b.rows.empty()) return refuse("block streaming needs a plan with one voice bank (this one has no voices)");
            LeafProgram lp;
            std::string why;
            if (!compile_leaf_program(b.shape, b.varying, b.literal_bits, b.alias, lp, &why, tracks)) return refuse(why);
            if (!lp.track_cols.empty()) {            // the staging: from the first declared slot to the highest one a table names
                if (env.track_from == 0xFFFFFFFFu || b.max_track_slot < env.track_from) return refuse("internal: a track voice without declared track slots");
                const uint64_t rows = (uint64_t)b.max_track_slot - env.track_from + 1;
                if (rows > STREAM_MAX_TRACK_ROWS)
                    return refuse("these track voices name " + std::to_string(rows) + " track rows (slots " + std::to_string(env.track_from) + " .. " + std::to_string(b.max_track_slot) +
                                  "); block streaming stages at most " + std::to_string(STREAM_MAX_TRACK_ROWS) + " per block");
                s.track_first = env.track_from;
                s.track_rows = std::max(s.track_rows, (uint32_t)rows);
            }
            if (sp.fused_sweep) return refuse("a sweep plan (a feedback loop that delays by a signal amount) together with compiled voices; block streaming has no sweep form with a leaf interpreter");
            for (const LeafInstr &in : lp.ins)
                for (int side = 0; side < 2; ++side) {
                    if ((side ? in.kb : in.ka) != LEAF_IN) continue;
                    const uint32_t slot = lp.input_slots[side ? in.b : in.a];
                    if (slot == 0) continue;
                    if (!env.inputs) return refuse("a leaf reads input slot " + std::to_string(slot) + "; block streaming feeds slot 0 only");
                    others.push_back(slot);
                }
            if (lp.result_kind == LEAF_IN && lp.input_slots[lp.result] != 0) {
                if (!env.inputs) return refuse("a leaf reads input slot " + std::to_string(lp.input_slots[lp.result]) + "; block streaming feeds slot 0 only");
                others.push_back(lp.input_slots[lp.result]);
            }
            StreamBank sb;
            sb.voices = (uint32_t)b.rows.size();
            sb.log2_p = b.log2_p;
            sb.to_ring = b.to_ring;
            sb.leaf = true;
            s.banks.push_back(sb);
            s.leaf_progs.push_back(std::move(lp));
            continue;
        }
        if (env.general) {
            if (b.jit || b.tracks || b.to_ws) return refuse("block streaming needs template voices (these are compiled or track voices)");
        } else if (b.general || b.jit || b.tracks || b.to_ws) {
            return refuse("block streaming needs balanced template voices (these are general, compiled or track voices)");
        }
        if (env.leaf_variant != 1) return refuse("block streaming with FR_BANK_LEAF=0");
        if (b.input_slot != 0) return refuse("block streaming feeds input slot 0; these voices read another slot");
        // FR_STREAM_GENERAL: a schedule bank -- general voices as the matcher cut them, balanced voices of 32 or 64 partials
        const bool schedule = env.general && (b.general || b.log2_p == 5 || b.log2_p == 6);
        if (!schedule && b.log2_p < 7) return refuse("block streaming needs voices of at least 128 partials (16 waves x one group of 8)");
        if (b.rows.empty()) return refuse("block streaming needs a plan with one voice bank (this one has no voices)");
        StreamBank sb;
        sb.voices = (uint32_t)b.rows.size();
        sb.log2_p = b.general ? 0 : b.log2_p;
        sb.to_ring = b.to_ring;
        sb.general = schedule;
        if (schedule) {
            for (uint32_t v = 0; v < sb.voices; ++v) {
                uint64_t leaves = 1ull << b.log2_p;
                if (b.general) {
                    std::string why;
                    if (!stream_schedule_ok(b.groups, b.group_off, v, &why)) return refuse("internal: a voice's schedule is malformed (" + why + ")");
                    leaves = stream_schedule_leaves(b.groups, b.group_off, v);
                }
                leaves = std::min<uint64_t>(leaves, UINT32_MAX);
                sb.max_leaves = std::max(sb.max_leaves, (uint32_t)leaves);
                s.general_voices.push_back((uint32_t)leaves);
            }
        }
        s.banks.push_back(sb);
        if (leaves) { s.leaf_progs.emplace_back(); s.leaf_progs.back().k = 0; }
    }
    if (!s.has_leaves()) s.leaf_progs.clear();       // (a plan without a leaf bank is what it has always been)
    if (!s.has_leaves()) s.track_rows = 0;
    // every workgroup of the launch must be resident at once, one per CU: chunks of >= 128 partials until the CUs are used
    const uint64_t max_wgs = stream_max_wgs(env.device_cus);
    if (!deal_stream_chunks(s.banks, max_wgs)) return refuse("block streaming serves at most one voice per CU (" + std::to_string(max_wgs) + " here)");
    for (uint32_t leaves : s.general_voices)         // one workgroup renders a schedule voice
        if (leaves > STREAM_GENERAL_MAX_LEAVES)
            return refuse("a voice of " + std::to_string(leaves) + " leaves; block streaming renders a voice of any partial count in one workgroup, at most " +
                          std::to_string(STREAM_GENERAL_MAX_LEAVES) + " leaves");
    uint32_t V = 0;
    for (const StreamBank &sb : s.banks) {
        V += sb.voices;
        s.chunks = std::max(s.chunks, 1u << (sb.log2_p - sb.chunk_log2));
    }
    s.voices = V;
    if (!voiceless) {
        s.chunk_log2 = s.banks[0].chunk_log2;
        s.bank_to_ring = s.banks[0].to_ring;
    }

    // the programs that do a block's work: the fused form (a feedback plan: level by level, then its row copies); a plan whose
    // programs are ONE level deep has no fused form because that level already is one
    std::vector<uint32_t> run;
    uint32_t first_copy = UINT32_MAX;                // position in `run` of the first row copy of a feedback plan
    if (sp.feedback) {
        for (uint32_t i = 0; i < sp.fused_count; ++i) run.push_back(sp.fused_first + i);
        first_copy = (uint32_t)run.size();
        for (uint32_t i = 0; i < sp.post_count; ++i) run.push_back(sp.post_first + i);
    } else if (sp.fused_count) {
        for (uint32_t i = 0; i < sp.fused_count; ++i) run.push_back(sp.fused_first + i);
    } else if (!sp.progs.empty()) {
        size_t levels = 0, only = 0;
        for (size_t l = 0; l + 1 < sp.level_first.size(); ++l)
            if (sp.level_first[l + 1] > sp.level_first[l]) { ++levels; only = l; }
        if (levels != 1 && !env.taps)
            return refuse("the plan has no fused form: a program's ring is read less than " + std::to_string(STREAM_BLOCK) +
                          " frames back (or the fused programs exceed the interpreter's budget)");
        if (levels == 1) {
            for (uint32_t i = sp.level_first[only]; i < sp.level_first[only + 1]; ++i) run.push_back(i);
        } else {                                     // FR_STREAM_TAPS: the level form itself, level by level, its row copies included
            for (size_t l = 0; l + 1 < sp.level_first.size(); ++l)
                for (uint32_t i = sp.level_first[l]; i < sp.level_first[l + 1]; ++i) run.push_back(i);
            s.levels = (uint32_t)levels;
        }
    }
    if (voiceless && run.empty()) return refuse("block streaming of a plan with neither voices nor programs");
    std::unordered_map<uint32_t, uint32_t> bank_ring_voice;   // ring -> voice whose frames it holds
    for (size_t i = 0; i < banks.size(); ++i)
        if (banks[i]->to_ring)
            for (uint32_t v = 0; v < s.banks[i].voices; ++v) bank_ring_voice[banks[i]->rows[v]] = s.banks[i].first_voice + v;
    std::unordered_map<uint32_t, uint32_t> stored_by;         // ring -> position in `run` of the program that stores it
    for (uint32_t k = 0; k < run.size(); ++k) {
        const StageProg &pg = sp.progs[run[k]];
        if (pg.dst_ring != 0xFFFFFFFFu) stored_by.emplace(pg.dst_ring, k);
        for (uint32_t i = 0; i < pg.n_instr; ++i) {
            const StageInstr &in = sp.instrs[pg.first_instr + i];
            if (in.op == S_STORE) stored_by.emplace(in.buf, k);
        }
    }
    constexpr uint32_t NONE = UINT32_MAX;
    // "voice" of a bus program: the segment after the last voice's.  A plan without a voice: voice_of holds a program's GROUP until
    // the groups are counted and dealt over the segments (below), and the bus has a number no group has
    const uint32_t BUS = voiceless ? UINT32_MAX - 1u : V;
    uint32_t groups = 0;
    const std::string whom = voiceless ? "program groups" : "voices", one_whom = voiceless ? "program group" : "voice";
    std::vector<uint32_t> voice_of(run.size(), NONE);
    const bool loops = env.loops && sp.feedback;              // FR_STREAM_LOOPS concerns a feedback plan's one-launch form
    const bool taps = env.taps && !sp.feedback;               // FR_STREAM_TAPS concerns every other plan
    // a read below a block of a ring that an EARLIER program of `run` stores binds the reader to the storer's voice (group): the
    // level behind a loop (loops), any level of a level form (taps)
    const bool follows = loops || taps;
    // FR_STREAM_SWEEP concerns a feedback plan too: S_READ_DYN of a ring the program stores itself (a sweep program), of a ring an
    // earlier program stores (admitted as `taps` admits it), and the _DYN ops inside a loop program of constant stride
    const bool sweeps = sweep && loops;
    const bool dyn_taps = taps || sweeps;
    std::vector<uint32_t> stride_of(run.size(), 0), width_of(run.size(), 0);
    // FR_STREAM_BUS: a program is a bus program when, at a delay below a block, it reads the bank rings of two or more voices
    // or a ring that an earlier bus program stores (a feedback plan's row copy of such a ring included)
    auto is_bus = [&](uint32_t k) {
        if (!env.bus) return false;
        const StageProg &pg = sp.progs[run[k]];
        uint32_t one = NONE;
        for (uint32_t i = 0; i < pg.n_instr; ++i) {
            const StageInstr &in = sp.instrs[pg.first_instr + i];
            const bool dyn_read = env.dyn && in.op == S_READ_DYN;   // (its offset may be below a block whatever its bound)
            if (dyn_read && !dyn_taps && bank_ring_voice.find(in.buf) == bank_ring_voice.end()) continue;   // (of a program's ring: refused below)
            if (!dyn_read && (in.op != S_READ || in.d_lo >= STREAM_BLOCK)) continue;
            auto bv = bank_ring_voice.find(in.buf);
            if (bv != bank_ring_voice.end()) {
                if (one != NONE && one != bv->second) return true;
                one = bv->second;
                continue;
            }
            auto st = stored_by.find(in.buf);
            if (st != stored_by.end() && st->second < k && voice_of[st->second] == BUS) return true;
            if (follows && st != stored_by.end() && st->second < k) {   // a tap behind a loop, a level behind a level: it follows the storer's voice
                if (one != NONE && one != voice_of[st->second]) return true;
                one = voice_of[st->second];
            }
        }
        return false;
    };
    // S_READ_INPUT, S_READ_INPUT_DYN without FR_STREAM_HISTORY (and whatever op the rule does not know): a stream keeps no input history
    auto no_history = [&](uint8_t op) {
        if (env.dyn)
            return std::string("a program uses ") + stage_op_name(op) +
                   " (a delayed read of an input row), which block streaming does not serve yet: a stream keeps no input history";
        return std::string("a program uses ") + stage_op_name(op) + (op == S_READ_INPUT ? " (a delayed read of the input row)" : " (a Delay by a signal amount)") +
               ", which block streaming does not serve yet";
    };
    // The reader of a ring that an earlier program stores, below a block: it follows the storer's voice (group) -- `mine` -- or, when
    // it already follows another, is refused ("" : it follows)
    auto follow = [&](uint32_t &mine, uint32_t theirs) {
        if (mine != NONE && mine != theirs)
            return "a program reads " + whom + " " + std::to_string(mine) + " and " + std::to_string(theirs) + " in the same block (a mix bus across " + whom +
                   "); each streamed program follows one " + one_whom;
        mine = theirs;
        return std::string();
    };
    uint64_t min_delay = UINT64_MAX;
    uint32_t n_dyn_reads = 0, n_dyn_steps = 0, n_hist_reads = 0, n_hist_dyn_reads = 0, n_short = 0, n_dyn_ring_reads = 0;
    for (uint32_t k = 0; k < run.size(); ++k) {
        const StageProg &pg = sp.progs[run[k]];
        const bool copy = k >= first_copy;
        const bool bus = is_bus(k);
        uint32_t mine = NONE;
        if (env.dyn && loops && !sweeps && stream_loop_stride(pg, sp.instrs.data() + pg.first_instr) != 0)   // the loop kernel's phases hoist frame-only loads
            for (uint32_t i = 0; i < pg.n_instr; ++i) {
                const uint8_t op = sp.instrs[pg.first_instr + i].op;
                if (op == S_READ_DYN || op == S_STEP_DYN || (env.history && op == S_READ_INPUT_DYN))
                    return refuse(std::string("a loop program uses ") + stage_op_name(op) +
                                  " (a Delay by a signal amount inside a feedback loop shorter than a block), which block streaming does not serve yet");
            }
        for (uint32_t i = 0; i < pg.n_instr; ++i) {
            const StageInstr &in = sp.instrs[pg.first_instr + i];
            switch (in.op) {
            case S_CONST: case S_STEP: case S_SUM2: case S_MUL: case S_DIV: case S_MOD: case S_MIN: case S_STORE: break;
            case S_READ_INPUT: case S_READ_INPUT_DYN:
                if (!env.history) return refuse(no_history(in.op));
                if (in.op == S_READ_INPUT_DYN) {                    // the amount is anything in [0, its proven bound]: the history holds them all
                    if (!env.dyn)
                        return refuse(std::string("a program uses ") + stage_op_name(in.op) + " (a Delay by a signal amount), which block streaming does not serve yet");
                    if (!sp.observed.empty())
                        return refuse("a Delay's bound was observed from input rows (FR_DELAY_OBSERVED); a stream stores no rows, so block streaming does not serve it");
                    // (its d_lo says "unbounded": the ordinary path keeps every input frame.  The planner leaves the amount's
                    // proven bound in `buf`, which no evaluator reads)
                    if (in.buf == 0xFFFFFFFFu)
                        return refuse("a program delays an input row by a signal amount without a proven bound; a stream's input history holds at most " +
                                      std::to_string(STREAM_HIST_MAX_FRAMES) + " frames");
                    ++n_hist_dyn_reads;
                    s.input_lookback = std::max<uint64_t>(s.input_lookback, in.buf);
                } else {
                    ++n_hist_reads;
                    s.input_lookback = std::max<uint64_t>(s.input_lookback, in.d_lo);
                }
                [[fallthrough]];                                    // its slot is streamed like an S_INPUT's; it reads no voice
            case S_INPUT:
                if (env.inputs && in.imm < sp.input_slots.size()) {
                    if (sp.input_slots[in.imm] != 0) others.push_back(sp.input_slots[in.imm]);
                    break;
                }
                if (in.imm >= sp.input_slots.size() || sp.input_slots[in.imm] != 0)
                    return refuse("a program reads input slot " + std::to_string(in.imm < sp.input_slots.size() ? sp.input_slots[in.imm] : in.imm) +
                                  "; block streaming feeds slot 0 only");
                break;
            case S_READ: {
                s.lookback = std::max<uint64_t>(s.lookback, in.d_lo);
                auto bv = bank_ring_voice.find(in.buf);
                if (bv != bank_ring_voice.end()) {
                    if (in.d_lo >= STREAM_BLOCK) break;             // an earlier block's frames: any voice's
                    if (bus) break;                                 // every voice of the block has finished
                    if (mine != NONE && mine != bv->second)
                        return refuse("a program reads voices " + std::to_string(mine) + " and " + std::to_string(bv->second) +
                                      " in the same block (a mix bus across voices); each streamed program follows one voice");
                    mine = bv->second;
                    break;
                }
                if (loops && in.d_lo != 0 && in.d_lo < STREAM_BLOCK) {   // a ring the program stores itself: a loop shorter than a block
                    auto st = stored_by.find(in.buf);
                    if (st != stored_by.end() && st->second == k) {
                        min_delay = std::min<uint64_t>(min_delay, in.d_lo);
                        ++n_short;
                        break;                                       // (its stride: stream_loop_stride, below)
                    }
                }
                if (bus && in.d_lo < STREAM_BLOCK) {                 // a ring an EARLIER program of the block stores: it has finished
                    auto st = stored_by.find(in.buf);
                    if (st != stored_by.end() && st->second < k) { ++n_short; break; }
                    return refuse("a program's ring is read " + std::to_string(in.d_lo) + " frames back; a streamed block needs delays of at least " +
                                  std::to_string(STREAM_BLOCK) + " frames");
                }
                if (copy && in.d_lo == 0) {                          // a row copy: after the program that stores the ring, on its voice
                    auto st = stored_by.find(in.buf);
                    if (st == stored_by.end() || voice_of[st->second] == NONE) return refuse("internal: a row copy of a ring no streamed program stores");
                    mine = voice_of[st->second];
                    ++n_short;
                    break;
                }
                if (follows && in.d_lo < STREAM_BLOCK) {             // a ring an EARLIER program stores, on one voice: the level behind a loop or a level
                    auto st = stored_by.find(in.buf);
                    if (st != stored_by.end() && st->second < k) {
                        const std::string two = follow(mine, voice_of[st->second]);
                        if (!two.empty()) return refuse(two);
                        min_delay = std::min<uint64_t>(min_delay, in.d_lo);
                        ++n_short;
                        break;
                    }
                }
                if (in.d_lo < STREAM_BLOCK)
                    return refuse("a program's ring is read " + std::to_string(in.d_lo) + " frames back; a streamed block needs delays of at least " +
                                  std::to_string(STREAM_BLOCK) + " frames");
                min_delay = std::min<uint64_t>(min_delay, in.d_lo);
                break;
            }
            case S_READ_DYN: case S_STEP_DYN: {
                if (!env.dyn)
                    return refuse(std::string("a program uses ") + stage_op_name(in.op) + " (a Delay by a signal amount), which block streaming does not serve yet");
                if (!sp.observed.empty())
                    return refuse("a Delay's bound was observed from input rows (FR_DELAY_OBSERVED); a stream stores no rows, so block streaming does not serve it");
                if (in.op == S_STEP_DYN) { ++n_dyn_steps; break; }  // touches no memory
                auto bv = bank_ring_voice.find(in.buf);
                if (bv == bank_ring_voice.end()) {
                    // FR_STREAM_TAPS: a ring an EARLIER program of `run` stores -- whatever the bound a read below a block, as of a voice
                    auto st = stored_by.find(in.buf);
                    if (sweeps && st != stored_by.end() && st->second == k) {   // FR_STREAM_SWEEP: a ring the program stores itself: a sweep program
                        // (imm: the amount's proven lower bound in frames; the planner refuses a sweep plan without one)
                        if (in.imm == 0) return refuse("internal: a program delays a ring it stores itself by a signal amount without a proven lower bound");
                        s.lookback = std::max<uint64_t>(s.lookback, in.d_lo);
                        ++n_dyn_reads; ++n_dyn_ring_reads;
                        min_delay = std::min<uint64_t>(min_delay, in.imm);
                        if (in.imm < STREAM_BLOCK) ++n_short;       // (it may reach into the block: its width, stream_sweep_width, below)
                        break;
                    }
                    if (!(dyn_taps && st != stored_by.end() && st->second < k))
                        return refuse("a program uses S_READ_DYN of a ring that a program stores (a Delay of a computed value by a signal amount, which may be 0 "
                                      "frames); block streaming serves signal delays of voices only");
                    s.lookback = std::max<uint64_t>(s.lookback, in.d_lo);
                    ++n_dyn_reads; ++n_dyn_ring_reads; ++n_short;
                    if (bus) break;                                 // every earlier program of the block has finished
                    const std::string two = follow(mine, voice_of[st->second]);
                    if (!two.empty()) return refuse(two);
                    min_delay = 0;                                  // (the amount may be 0 frames)
                    break;
                }
                s.lookback = std::max<uint64_t>(s.lookback, in.d_lo);
                ++n_dyn_reads;
                if (bus) break;                                     // every voice of the block has finished
                if (mine != NONE && mine != bv->second)
                    return refuse("a program reads voices " + std::to_string(mine) + " and " + std::to_string(bv->second) +
                                  " in the same block (a mix bus across voices); each streamed program follows one voice");
                mine = bv->second;
                break;
            }
            default: return refuse(no_history(in.op));
            }
            if (in.dst >= STAGE_REGS || in.a >= STAGE_REGS || in.b >= STAGE_REGS) return refuse("a program needs more registers than the streamed interpreter has");
        }
        if (pg.result_reg >= STAGE_REGS) return refuse("a program needs more registers than the streamed interpreter has");
        // FR_STREAM_SWEEP: a sweep program's width stands where a loop program's stride stands; at width 64 no read reaches into a
        // block and the program runs lane = frame, like a comb of 64 frames
        const uint32_t width = sweeps ? stream_sweep_width(pg, sp.instrs.data() + pg.first_instr) : 0u;
        if (width >= 1 && width < STREAM_BLOCK) stride_of[k] = width_of[k] = width;
        if (loops && (width_of[k] != 0 || (stride_of[k] = stream_loop_stride(pg, sp.instrs.data() + pg.first_instr)) != 0)) {
            const uint32_t n_ld = stream_loop_loads(pg, sp.instrs.data() + pg.first_instr);
            const size_t n_st = stream_stored_rings(pg, sp.instrs.data() + pg.first_instr).size();
            if (n_ld > STREAM_LOOP_LOADS)
                return refuse("a loop program has " + std::to_string(n_ld) + " frame-only loads; block streaming serves at most " + std::to_string(STREAM_LOOP_LOADS));
            if (n_st > STREAM_LOOP_STORES)
                return refuse("a loop program stores " + std::to_string(n_st) + " rings; block streaming serves at most " + std::to_string(STREAM_LOOP_STORES));
            if (sweeps && width_of[k] == 0)                          // (a loop program of constant stride with a _DYN op: the sweep walk runs it)
                for (uint32_t i = 0; i < pg.n_instr; ++i) {
                    const uint8_t op = sp.instrs[pg.first_instr + i].op;
                    if (op == S_READ_DYN || op == S_STEP_DYN || op == S_READ_INPUT_DYN) s.sweep_loops = true;
                }
        }
        // (reads no voice at a short delay: any one voice, the same every time; without a voice: it follows nobody and opens a group)
        voice_of[k] = bus ? BUS : mine != NONE ? mine : voiceless ? groups++ : run[k] % V;
    }
    if (s.input_lookback > STREAM_HIST_MAX_FRAMES)
        return refuse("a program reads an input row " + std::to_string(s.input_lookback) + " frames back; a stream's input history holds at most " +
                      std::to_string(STREAM_HIST_MAX_FRAMES) + " frames");
    std::sort(others.begin(), others.end());
    others.erase(std::unique(others.begin(), others.end()), others.end());
    if (1 + others.size() > STREAM_MAX_INPUTS)
        return refuse(std::string(s.has_leaves() ? "the leaves and the programs read " : "the programs read ") + std::to_string(1 + others.size()) + " distinct input slots (slot 0 included); block streaming feeds at most " +
                      std::to_string(STREAM_MAX_INPUTS));
    // each output row: one assigned program, or the bank itself
    std::vector<uint32_t> writers(env.n_slots, 0);
    auto writes = [&](int64_t row) { if (row >= 0 && row < (int64_t)env.n_slots) ++writers[(size_t)row]; return row < (int64_t)env.n_slots; };
    for (const BankLaunch *bp : banks)
        if (!bp->to_ring)
            for (uint32_t row : bp->rows)
                if (!writes(row)) return refuse("a voice writes output row " + std::to_string(row) + " of " + std::to_string(env.n_slots));
    for (uint32_t k = 0; k < run.size(); ++k)
        if (!writes(sp.progs[run[k]].out_row)) return refuse("a program writes output row " + std::to_string(sp.progs[run[k]].out_row) + " of " + std::to_string(env.n_slots));
    for (uint32_t r = 0; r < env.n_slots; ++r)
        if (writers[r] != 1)
            return refuse("output row " + std::to_string(r) + " is written by " + std::to_string(writers[r]) + " streamed programs or voices (exactly one is needed)");
    if (voiceless) {                                          // group g runs in segment g % segments, the bus programs behind the last segment
        s.segments = (uint32_t)std::min<uint64_t>(groups, max_wgs);
        if (s.segments == 0) return refuse("internal: a plan without a voice whose programs are all bus programs");
        for (uint32_t &v : voice_of) v = v == BUS ? s.segments : v % s.segments;
        V = s.segments;
    }
    s.voice_first.assign(V + 2, 0);
    for (uint32_t k = 0; k < run.size(); ++k) ++s.voice_first[voice_of[k] + 1];
    for (uint32_t v = 0; v <= V; ++v) s.voice_first[v + 1] += s.voice_first[v];
    s.progs.resize(run.size());
    s.loop_stride.resize(run.size());
    s.sweep_width.resize(run.size());
    std::vector<uint32_t> at(s.voice_first.begin(), s.voice_first.end() - 1);
    for (uint32_t k = 0; k < run.size(); ++k) {                                      // (stable: the order of `run` inside a voice)
        s.loop_stride[at[voice_of[k]]] = stride_of[k];
        s.sweep_width[at[voice_of[k]]] = width_of[k];
        s.progs[at[voice_of[k]]++] = run[k];
    }
    s.min_ring_delay = min_delay == UINT64_MAX ? 0 : min_delay;
    s.dyn_reads = n_dyn_reads;
    s.dyn_steps = n_dyn_steps;
    s.short_reads = n_short;
    s.dyn_ring_reads = n_dyn_ring_reads;
    s.hist_reads = n_hist_reads;
    s.hist_dyn_reads = n_hist_dyn_reads;
    s.input_slots.insert(s.input_slots.end(), others.begin(), others.end());
    s.servable = true;
    return s;
}

// ---- the launch rule ----------------------------------------------------------------------------------------------------------
inline const char *stream_kernel_name(StreamKernel k) {
    static const char *const names[] = {"", "bank_stream_kernel", "bank_stream_prog_kernel", "bank_stream_bus_kernel", "bank_stream_in_kernel",
                                        "bank_stream_banks_kernel", "bank_stream_loops_kernel", "bank_stream_general_kernel", "bank_stream_dyn_kernel"};
    if (k == StreamKernel::hist) return "bank_stream_hist_kernel";   // (not the value after dyn: that one has no name)
    if (k == StreamKernel::fx) return "bank_stream_fx_kernel";       // (nor the value after hist)
    if (k == StreamKernel::store) return "bank_stream_store_kernel";
    if (k == StreamKernel::store_fx) return "bank_stream_store_fx_kernel";
    if (k == StreamKernel::sweep) return "bank_stream_sweep_kernel";
    if (k == StreamKernel::sweep_fx) return "bank_stream_sweep_fx_kernel";
    if (k == StreamKernel::sweep_store) return "bank_stream_sweep_store_kernel";
    if (k == StreamKernel::sweep_store_fx) return "bank_stream_sweep_store_fx_kernel";
    if (k == StreamKernel::leaf) return "bank_stream_leaf_kernel";
    if (k == StreamKernel::leaf_store) return "bank_stream_leaf_store_kernel";
    if (k == StreamKernel::track) return "bank_stream_track_kernel";
    if (k == StreamKernel::track_store) return "bank_stream_track_store_kernel";
    return names[(uint32_t)k < sizeof names / sizeof names[0] ? (uint32_t)k : 0];
}

inline bool stream_kernel_by_plan(StreamKernel k) { return k >= StreamKernel::in; }

struct StreamLaunch {
    StreamKernel kernel = StreamKernel::none;
    bool rows_doorbell = false;      // the doorbell is n_rows rows (BankStreamInCtl / BankStreamInDev); else one row (BankStreamCtl / BankStreamDev)
    uint32_t n_rows = 1;             // the rows a block brings: StreamPlan::input_slots, in that order (one row: slot 0)
    bool own_instrs = false;         // the programs run from the stream's own copy of their instructions (S_INPUT by row, store slots)
    bool bank_table = false;         // the banks travel as a table (StreamBanksArgs), voices numbered globally
    bool schedule_table = false;     // ... and the schedule banks' schedules next to it (StreamGeneralArgs)
    uint32_t max_stride = 0, max_loads = 0, max_stores = 0;   // the loop programs' largest stride, load count and store-slot count
    uint32_t workgroups = 0;
    uint64_t hist_cap = 0;           // the history's frames per streamed row, a power of two >= 64 (0: the kernel keeps none)
    bool by_plan = false;            // the plan alone decides the kernel: fr_plan_json names it before any launch (stream_kernel_by_plan)
};

// The path fr_stream_begin takes: true = the program path (plan_stream, stream_launch), false = the plain path (one balanced bank
// that writes the rows: plain_stream_launch).  FR_STREAM_BANKS: several banks take the program path even without programs and
// rings; FR_STREAM_GENERAL: so does a bank that the option may serve by schedule -- general voices, voices below 128 partials;
// FR_STREAM_STORE (StreamEnv::store): every plan, also the one balanced bank that writes rows.
inline bool stream_path(const StagedPlan &sp, const std::vector<const BankLaunch *> &banks, const StreamEnv &env) {
    const bool by_schedule = env.general && std::any_of(banks.begin(), banks.end(), [](const BankLaunch *b) { return b->general || b->log2_p < 7; });
    const bool by_leaves = env.leaves && std::any_of(banks.begin(), banks.end(), [](const BankLaunch *b) { return b->jit; });   // FR_STREAM_LEAVES: a compiled bank
    return env.programs && (!sp.progs.empty() || sp.uses_rings() || (env.banks && banks.size() > 1) || by_schedule || by_leaves || env.store);
}

// The launch of a servable plan of the program path.  The one cascade: hist > dyn > general > loops > banks > in > bus > prog.
// dyn -- a plan with a Delay by a signal amount (StreamPlan::has_dyn) -- is the general kernel's composition and takes the
// schedule table only when the plan has schedule banks; hist -- a plan with a delayed read of an input row
// (StreamPlan::has_hist), and no other -- is dyn's composition with the history of the streamed rows.  Ahead of the cascade: fx --
// a plan without a voice (StreamPlan::voices == 0, FR_STREAM_EFFECTS), and no other --: one workgroup per segment, no bank and
// no schedule table, and always the history (at least a block per row also when nothing reads it: n_rows x 64 floats spare an
// eleventh kernel).  On top of both: the store forms (StreamPlan::store, FR_STREAM_STORE) -- store for every plan with voices,
// whatever the cascade would have chosen, store_fx for a plan without; the history is at least a block per row in both, and
// n_rows counts the plan's slots (a store-mode stream may stream more: streamstore.hpp stream_store_slots, the engine's launch).
// In front of everything: the sweep forms (StreamPlan::has_sweep, FR_STREAM_SWEEP) -- sweep is the hist form and the sweep walk,
// sweep_fx the fx form, sweep_store and sweep_store_fx the store forms with it; the history, the tables and n_rows are those of the
// form underneath.  And the leaf forms (StreamPlan::has_leaves, FR_STREAM_LEAVES; the rule refuses a sweep plan with a leaf bank):
// leaf is the hist form -- history, both tables -- with the leaf interpreter, leaf_store the store form with it.  In front of
// those, the track forms (StreamPlan::has_tracks, FR_STREAM_TRACKS): the leaf forms whose leaves read the block's staged matrix.
inline StreamLaunch stream_launch(const StagedPlan &sp, const StreamPlan &s) {
    StreamLaunch l;
    const bool fx = s.voices == 0;
    l.kernel = s.has_tracks() ? (s.store ? StreamKernel::track_store : StreamKernel::track)
               : s.has_leaves() ? (s.store ? StreamKernel::leaf_store : StreamKernel::leaf)
               : s.has_sweep() ? (s.store ? (fx ? StreamKernel::sweep_store_fx : StreamKernel::sweep_store) : fx ? StreamKernel::sweep_fx : StreamKernel::sweep)
               : s.store ? (fx ? StreamKernel::store_fx : StreamKernel::store) : fx ? StreamKernel::fx : s.has_hist() ? StreamKernel::hist : s.has_dyn() ? StreamKernel::dyn : s.has_general() ? StreamKernel::general : s.has_loops() ? StreamKernel::loops
               : s.banks.size() > 1 ? StreamKernel::banks : s.input_slots.size() > 1 ? StreamKernel::in : s.bus_programs() ? StreamKernel::bus : StreamKernel::prog;
    l.rows_doorbell = l.own_instrs = l.by_plan = stream_kernel_by_plan(l.kernel);
    l.bank_table = !fx && l.kernel >= StreamKernel::banks;   // (fx: also store_fx)
    l.schedule_table = !fx && (l.kernel == StreamKernel::general || (l.kernel >= StreamKernel::dyn && s.has_general()));
    l.hist_cap = fx || s.store || l.kernel == StreamKernel::hist || l.kernel == StreamKernel::sweep || l.kernel == StreamKernel::leaf || l.kernel == StreamKernel::track ? stream_hist_cap(s.input_lookback) : 0;
    l.n_rows = l.rows_doorbell ? (uint32_t)s.input_slots.size() : 1u;
    for (size_t i = 0; i < s.progs.size(); ++i) {    // (the tiles' fill is counted from the plan's instructions; the store slots are the stored rings)
        if (!s.loop_stride[i]) continue;
        const StageProg &pg = sp.progs[s.progs[i]];
        l.max_stride = std::max(l.max_stride, s.loop_stride[i]);
        l.max_loads = std::max(l.max_loads, stream_loop_loads(pg, sp.instrs.data() + pg.first_instr));
        l.max_stores = std::max(l.max_stores, (uint32_t)stream_stored_rings(pg, sp.instrs.data() + pg.first_instr).size());
    }
    l.workgroups = fx ? s.segments : s.workgroups();
    return l;
}

// The plain path's launch: one bank of `voices` balanced voices of 1 << log2_p partials (log2_p >= 7), a one-row doorbell, no
// tables; `bank` gets the chunks.  False: more than max_wgs workgroups (the caller's limit: the plain path counts an unknown CU
// count as one CU, stream_max_wgs() as the kernel's limit).
inline bool plain_stream_launch(uint32_t voices, uint32_t log2_p, uint64_t max_wgs, StreamBank &bank, StreamLaunch &l) {
    std::vector<StreamBank> one(1);
    one[0].voices = voices; one[0].log2_p = log2_p;
    if (!deal_stream_chunks(one, max_wgs)) return false;
    bank = one[0];
    l = StreamLaunch{};
    l.kernel = StreamKernel::plain;
    l.workgroups = voices << (log2_p - bank.chunk_log2);
    return true;
}

}  // namespace fr
