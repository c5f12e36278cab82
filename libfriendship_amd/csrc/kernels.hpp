// kernels.hpp -- launch interface between the host engine and the gfx950 kernels.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace fr {

// One external input slot's stored history (reference.rs:25 `inputs[slot]`), device resident.
// value(t) = t < base ? 0 : t < len ? data[t - base] : 0.   `base` is the zero prefix left by a seek.
struct DevInput {
    const float *data;
    uint64_t base;
    uint64_t len;
};

// Lowered node as the device sees it: {op, a, b, depth} (graph.hpp FlatNode), 16 bytes.
struct DevNode {
    uint32_t op, a, b, depth;
};

struct PullArgs {
    const DevNode *nodes;
    const uint32_t *outputs;   // [n_slots] root node per output slot
    const DevInput *inputs;    // [n_inputs]
    uint32_t n_inputs;
    float *out;                // [n_slots, n_times] row-major
    uint32_t n_slots;
    uint64_t n_times;
    uint64_t idx;
    uint64_t first;            // first linear (slot*n_times + t) element of this launch
    uint64_t count;            // elements in this launch
    uint32_t sparkle;          // FR_SEMANTICS_SPARKLE: Minimum / Delay as SparkleRenderer computes them (kernels.hip prim_min)
    uint32_t *st_node;         // pull stack, [depth][count]
    uint64_t *st_time;
    float *st_val;
};
hipError_t launch_pull(const PullArgs &a, hipStream_t s);

// Fused oscillator bank (see kernels.hip): out[v][t] = balanced Sum2 tree over P partials of
// amp * parabolic_sine(Modulo(time[t] * w, 1)).
struct BankArgs {
    const float2 *params;      // [n_voices][P] {w, -4*amp}
    // Window frame ti (0 <= ti < n_times) reads the time-carrying input as
    //   ti < time_skip ? 0 : (ti - time_skip < time_valid ? time[ti - time_skip] : 0)
    const float *time;         // stored history of the time slot, starting at window frame time_skip (may be null)
    uint64_t time_skip;        // leading window frames that precede the stored history (zero after a seek)
    uint64_t time_valid;       // stored frames available from `time`; beyond -> 0
    // Voice v writes window frame ti to out[rows[v] * out_stride + (ring_mask ? (ring_t0 + ti) & ring_mask : ti)]
    float *out;
    const uint32_t *rows;      // [n_voices] destination row of each voice
    uint64_t out_stride;       // floats between destination rows
    uint64_t ring_mask;        // 0: rows are linear windows; else rows are rings of ring_mask + 1 floats
    uint64_t ring_t0;          // absolute frame of window frame 0 (ring addressing)
    uint32_t n_voices;
    uint32_t log2_p;           // P = 1 << log2_p
    uint64_t n_times;          // window length in frames
    uint32_t fast_ok;          // every w in [0, 2^32]: the non-negative fast path may be used
    uint32_t chunk_log2;       // partials per workgroup = 1 << chunk_log2 (5..13, <= log2_p); from bank_shape
    uint32_t frames_per_lane;  // 1, 2 or 4; from bank_shape
    uint32_t waves_per_group;  // 4 or 8; from bank_shape
    uint32_t small_call;       // from bank_shape.  1: lanes-over-partials kernel (calls of <= 2 frames).  2: the short-call
                               // kernel: too few (voice, tile) pairs to fill the chip, so every voice is split into chunks over
                               // several workgroups of 4..16 waves, parameters staged through LDS, chunk sums combined by the
                               // last workgroup to arrive (`tickets`) -- one launch
    uint32_t voices_per_wave;  // > 0: many small voices (<= 256 partials): a wave sums WHOLE voices, this many in a row, for one
                               // tile of frames -- no LDS, no barriers, the time values stay in registers (bank_multi_kernel)
    uint32_t leaf_variant;     // 0 = product-form leaves; 1 = FMA-form leaves + zero-sign repair (same bits, faster)
    float *hist_dst;           // if non-null: the kernel also copies time[0..time_valid) here (input-history append)
    float *ws;                 // [P >> chunk_log2][n_voices][n_times] partial sums; unused when one chunk
    // Row-completion flags for the host entry point (fr_fill_buffer streaming its output, engine.cpp): when host_flags is
    // set (time-major kernel, one chunk per voice only), the workgroup that finishes the LAST tile of voice v -- counted
    // in row_done[v], zero between launches -- stores flag_value to host_flags[rows[v]] (mapped host memory) after every
    // output store of the voice has been acknowledged: the host may then read that row while other voices still compute.
    uint32_t *row_done;
    uint32_t *host_flags;
    uint32_t flag_value;
    uint32_t *tickets;         // small_call == 2 with chunks: [n_voices][tiles] arrival counters, BANK_TICKET_STRIDE words
                               // apart, all zero between launches
    // general voices (launch_gbank): groups[i] = log2(item leaves, <= 11) | merges_after << 4; params = the items'
    // {w, -4*amp} pairs in order, items of < 8 leaves padded to 8 pairs; voice v owns items
    // [group_off[2v], group_off[2v+2]) and its parameters start at pair 8 * group_off[2v+1]
    const uint32_t *groups;
    const uint32_t *group_off;
};
constexpr uint32_t BANK_TICKET_STRIDE = 32;

// ---- block streaming (fr_stream_*, engine.cpp): ONE resident launch renders block after block -------------------------
// What a real-time host pays per 64-frame block through fr_fill_buffer is the launch path (~12 us from enqueue to first
// wave on this stack, profiles/r02_host_short_blocks.txt), not the 1.3 us of arithmetic.  Here the kernel is launched once
// and stays: the host rings a doorbell in mapped pinned memory, workgroup 0 sees it, copies the block's input row into
// device memory and releases the other workgroups; each renders its (voice, chunk) exactly as bank_short_kernel does, the
// chunk sums meet through the same tickets, finished rows go straight to mapped host memory and the workgroup that
// completes the last voice writes the block's sequence number back.  No workgroup ever waits for another one's result
// (tickets: the last arriver does the work), and every polling loop is bounded on the wall clock: without a doorbell for
// BANK_STREAM_IDLE_MS (the one number, quoted in friendship_render.h as FR_STREAM_IDLE_MS) the kernel ends itself, so a
// host that dies leaves no spinning GPU behind.
struct BankStreamCtl {        // mapped pinned host memory
    // host -> device.  The doorbell IS the block's input row: word i = row[i] (low half) | tag (high half), tag = the block's
    // sequence number << 8 | frames in the block (1..64; 0xFFFFFFFF = stop), written with one 8-byte store each.  Lane i of
    // workgroup 0 polls word i: a word whose tag is new carries its value with it (8-byte loads do not tear), so one trip
    // across PCIe brings both the news and the data (three dependent trips -- doorbell, length, row -- cost 5 us more).
    unsigned long long row[64];
    uint32_t done;            // device -> host: tag of the last finished block
    uint32_t alive;           // device -> host: 1 while the kernel is resident, 0 once it has ended
    uint32_t pad1[14];
};
struct BankStreamDev {        // device memory
    uint32_t seq;             // the doorbell, republished by workgroup 0 (0xFFFFFFFF = stop)
    uint32_t n_times;
    uint32_t voices_done;
    uint32_t pad[13];
    float row[64];
};
constexpr uint32_t BANK_STREAM_STOP = 0xFFFFFFFFu;
constexpr uint32_t BANK_STREAM_WGS = 256;      // most workgroups a stream may use (the caller also checks the device's CU count: all must be resident)
constexpr uint32_t BANK_STREAM_IDLE_MS = 2000; // the resident launch ends itself after this long without a block
// `a`: as for the short-call kernel (small_call == 2, 16 waves, chunk_log2 chosen so that voices * chunks <= the CUs of the device),
// out = device pointer of the mapped [n_voices][64] host result (out_stride = 64), ws / tickets allocated for 64 frames.
// Launches exactly n_voices * chunks workgroups.  idle_ms: 0 = BANK_STREAM_IDLE_MS.  (The entry: launch_bank_stream, below.)
uint64_t bank_blocks(const BankArgs &a);
hipError_t launch_bank(const BankArgs &a, hipStream_t s);
hipError_t launch_gbank(const BankArgs &a, hipStream_t s);   // voices that are arbitrary Sum2 trees (schedule form)

// ---- staged evaluator -------------------------------------------------------------------------------
// A cut node (a value some Delay reads back in time, or an output) is computed per frame by a small
// register program over: constants, inputs at t, and ring reads of other cut nodes at t - d.
enum StageOp : uint8_t {
    S_CONST = 0,       // dst = bits(imm)
    S_INPUT = 1,       // dst = input[imm] at t
    S_READ = 2,        // dst = t >= d ? ring[buf][(t - d) & mask] : 0          d = {lo, hi}
    S_READ_INPUT = 3,  // dst = t >= d ? input[imm] at t - d : 0
    S_STEP = 4,        // dst = t >= d ? bits(imm) : 0                           Delay of a constant
    S_SUM2 = 5, S_MUL = 6, S_DIV = 7, S_MOD = 8, S_MIN = 9,   // dst = a op b    (kernels.hip: prim_binop is the semantics, STAGE_ARITH_CASES
                                                              //  the cases of all five device interpreters)
    S_STORE = 10,      // ring[buf][t & mask] = a        (fused form: an inlined cut node still feeds its ring)
    // Delay with a signal amount (register a, evaluated at t): frames = amount -> u64 as reference.rs:200-211
    // (>= 2^64 -> output 0; negative/NaN -> 0 frames; else floor), then as the constant forms.  d_lo = proven bound.
    S_READ_DYN = 11,        // dst = ring[buf] at t - frames         (imm: 0, but in the fused programs of a sweep plan -- FR_LOOP_DYN,
                            //  StagedPlan::fused_sweep != 0 -- the amount's proven LOWER bound in frames; no evaluator reads it)
    S_READ_INPUT_DYN = 12,  // dst = input[imm] at t - frames         (buf = the amount's proven bound, 0xFFFFFFFF: none; no evaluator reads it)
    S_STEP_DYN = 13,        // dst = t >= frames ? bits(imm) : 0
};
struct StageInstr {    // 16 bytes
    uint8_t op, dst, a, b;
    uint32_t imm;
    uint32_t buf;      // ring index (S_READ)
    uint32_t d_lo;     // delay frames, low 32 bits (delays >= 2^32 frames are not staged)
};
struct StageProg {
    uint32_t first_instr, n_instr;
    uint32_t result_reg;
    uint32_t dst_ring;     // ring to store into, or 0xFFFFFFFF
    int32_t out_row;       // output row to store into (frames >= idx), or -1
    uint32_t n_loads;      // the first n_loads instructions are loads/constants with no register operands: the kernel
                           // issues them back to back so their memory latencies overlap (<= STAGE_MAX_HOISTED)
    uint32_t pad[2];
};
constexpr int STAGE_REGS = 48;
constexpr uint32_t STAGE_INLINE_INPUTS = 8;
constexpr uint32_t STAGE_MAX_HOISTED = 24;
struct StageArgs {
    const StageInstr *instrs;
    const StageProg *progs;    // programs of this level
    uint32_t n_progs;
    float *rings;              // [n_rings][ring_mask + 1]
    uint64_t ring_mask;
    const DevInput *inputs;    // [n_inputs] in device memory, used when n_inputs > STAGE_INLINE_INPUTS
    DevInput inline_inputs[8]; // the usual case: the table travels in the kernel arguments (no copy, no sync)
    uint32_t n_inputs;
    float *out;                // [n_slots, n_times] of the call
    uint64_t n_times;
    uint64_t idx;              // first frame of the call
    uint64_t w0;               // first frame of the window computed now (<= idx)
    uint64_t w_len;            // window length
    uint64_t stride;           // 0: thread wi computes frame w0 + wi; else the frames w0 + wi + k * stride inside the window, in order
                               // (StagedPlan::fused_stride: a long steady call of the fused form in ONE launch)
    uint32_t sparkle;          // FR_SEMANTICS_SPARKLE
    uint32_t carry_only;       // strided launches: every read of a ring that this launch stores comes from the carry (below), so
                               // a stride's stores need not be in memory before the next stride starts
    uint32_t use_carry;        // the programs carry annotations (feedback plans): the launch gets the carry's LDS
    uint32_t tile;             // 0: stage_kernel.  Else (callplan.hpp loop_tile, FR_LOOP_TILES) stage_tile_kernel: one wave per program
                               // renders the window in tiles of this many frames -- a multiple of `stride`, at most STAGE_TILE_FRAMES
    uint32_t sweep;            // launch_stage_sweep only (callplan.hpp loop_sweep, FR_LOOP_DYN): frames per sweep, 1..STAGE_SWEEP_MAX
};
// stage_tile_kernel's LDS: the tile's frame-only loads and its stores as [slot][frame in tile]
constexpr uint32_t STAGE_TILE_FRAMES = 256, STAGE_TILE_LOADS = 16, STAGE_TILE_STORES = 12;
// Carry (feedback plans, stage.cpp): a strided thread that reads back, `stride` frames later, what it stored to a ring in its
// previous iteration need not go through memory for it -- a dependent L2 round trip per iteration, all there is to a one-sample
// loop.  S_STORE.imm = carry slot + 1 keeps the stored value (double-buffered by iteration parity, so that the order of stores
// and reads inside an iteration does not matter); S_READ.imm = carry slot + 1 (only where d_lo == the launch's stride and the
// ring is one the program stores) takes it from there, except in the thread's first iteration of the launch.  0 = no carry.
constexpr uint32_t STAGE_CARRY = 8;
hipError_t launch_stage(const StageArgs &a, hipStream_t s);
// Sweeps (FR_LOOP_DYN): stage_sweep_kernel, one workgroup of 64 * ceil(sweep / 64) threads per program.  For base = 0, sweep,
// 2 sweep ... < w_len, thread f < min(sweep, w_len - base) runs the whole program for frame w0 + base + f with stage_kernel's
// arithmetic and stores; the sweep's stores are then waited for and a workgroup barrier passed before any thread starts the next
// sweep.  Valid when every read of a ring that the program stores reaches at least `sweep` frames back (StagedPlan::fused_sweep);
// `stride`, `carry_only`, `use_carry` and `tile` must be 0.  Ring indices are masked, whatever the amount.
constexpr uint32_t STAGE_SWEEP_MAX = 256;
hipError_t launch_stage_sweep(const StageArgs &a, hipStream_t s);

// ---- block streaming of plans with programs (FR_STREAM_PROGRAMS, streamplan.hpp) ----------------------------------------
// bank_stream_prog_kernel: bank_stream_kernel with an epilogue.  Wave 0 of the workgroup that finishes voice v holds the
// voice's frames head + lane; it stores them to the voice's ring (bank_to_ring; else to the voice's output row), then
// interprets progs[voice_first[v] .. voice_first[v + 1]) in order, lane = frame, the interpreter's registers in LDS: S_INPUT
// is the block's row, ring reads and stores go through L2 (relaxed agent-scope atomics: the finisher of a voice changes CU
// from block to block), output rows go to the mapped host buffer.  Ring and row stores alike are acknowledged before the
// voice is counted in, so block k's done tag implies that every ring store of block k has landed.  `head` advances by each
// block's length inside the launch; the host launches again for a block that does not continue the previous one.
struct StreamProgArgs {
    const StageInstr *instrs;      // the plan's instructions (StageProg::first_instr indexes them)
    const StageProg *progs;        // the streamed programs, voice by voice
    const uint32_t *voice_first;   // [n_voices + 2] into progs; the last segment: the bus programs (bank_stream_bus_kernel only)
    float *rings;                  // [n_rings][ring_mask + 1]
    uint64_t ring_mask;
    uint32_t n_rings;
    uint32_t n_rows;               // output rows of the mapped host result ([n_rows][64])
    uint64_t head;                 // absolute frame of the first block's first frame
    uint32_t bank_to_ring;         // BankArgs::rows are ring indices
    uint32_t sparkle;              // FR_SEMANTICS_SPARKLE
};
// bank_stream_bus_kernel (FR_STREAM_BUS): bank_stream_prog_kernel, and the wave whose voices_done ticket is the block's last
// (n_voices - 1) interprets progs[voice_first[n_voices] .. voice_first[n_voices + 1]) -- the bus programs, which read several
// voices of the same block -- before it resets the counter and stores the done tag.  Every voice acknowledged its ring and
// row stores before its ticket, the last arriver loads after its own: no wait, no acquire or release, no new polling loop.

// bank_stream_in_kernel (FR_STREAM_INPUTS): bank_stream_bus_kernel's work -- per-voice programs, then the bus programs in the
// block's last arriver, a segment that may be empty -- for programs that read control rows: up to BANK_STREAM_ROWS input slots
// at the current frame.  The doorbell is the block's `n_rows` rows (launch-uniform, 1..BANK_STREAM_ROWS; row 0 is the time
// slot's): every word carries its sample and the block's tag as in BankStreamCtl, wave 0 of workgroup 0 has the loads of all
// the rows in flight together in each look, and the block has arrived when every lane of every row holds the same new tag --
// one trip across PCIe however many rows there are.  It republishes the rows to BankStreamInDev::rows and releases the other
// workgroups as bank_stream_kernel does.  S_INPUT's operand is the ROW: `instrs` is the stream's own copy of the programs'
// instructions with every S_INPUT's imm rewritten to its streamed row (engine.cpp begin_program_stream); row 0 stays the `t`
// the finishing wave holds in a register, the others are loaded with the program's leading loads.
constexpr uint32_t BANK_STREAM_ROWS = 8;
struct BankStreamInCtl {      // mapped pinned host memory
    unsigned long long rows[BANK_STREAM_ROWS][64];   // host -> device: word i of row j = rows[j][i] (low half) | tag (high half)
    uint32_t done;            // device -> host: tag of the last finished block
    uint32_t alive;           // device -> host: 1 while the kernel is resident, 0 once it has ended
    unsigned long long tracks;   // host -> device (the track forms, StreamTrackArgs): the block's slot limit | staged rows << 32,
                                 // written before the block's doorbell words; 0: the block brought no matrix
    uint32_t pad1[12];
};
static_assert(sizeof(BankStreamInCtl) == BANK_STREAM_ROWS * 64 * 8 + 64 && offsetof(BankStreamInCtl, tracks) % 8 == 0, "the control block of rows keeps its size");
struct BankStreamInDev {      // device memory
    uint32_t seq;             // the doorbell, republished by workgroup 0 (0xFFFFFFFF = stop)
    uint32_t n_times;
    uint32_t voices_done;
    uint32_t pad[13];
    float rows[BANK_STREAM_ROWS][64];
};

// bank_stream_banks_kernel (FR_STREAM_BANKS): bank_stream_in_kernel's work for a plan of 2..BANK_STREAM_BANKS bank launches --
// voices of several partial counts, voices that write rows next to voices that feed rings -- in ONE resident launch.  The bank
// table is a by-value launch argument (kernarg, then SGPRs: nothing is uploaded); a workgroup finds its bank with at most
// n_banks - 1 uniform compares of its index against first_wg, once, before the block loop, and takes voice, chunk and chunk
// size from that bank's fields.  Voices are numbered globally (banks in table order, then voices in bank order): the chunk
// sums meet at ws + voice * 64 + chunk * (V_total * 64), V_total * (largest chunk count) * 64 floats in all, one ticket per
// global voice; StreamProgArgs::voice_first is indexed by the global voice and the block is done when V_total voices are.
// BankArgs gives n_voices = V_total, out, ws and tickets; its params, rows, log2_p, chunk_log2 and fast_ok, and
// StreamProgArgs::bank_to_ring, are not read (each bank has its own).
constexpr uint32_t BANK_STREAM_BANKS = 8;
struct StreamBanksArgs {
    uint32_t n_banks;
    struct Bank {
        const float2 *params;      // [n_voices][1 << log2_p] {w, -4*amp}
        const uint32_t *rows;      // [n_voices] destination of each voice: a ring (to_ring) or an output row
        uint32_t first_wg, first_voice, n_voices, log2_p, chunk_log2, fast_ok, to_ring;
    } bank[BANK_STREAM_BANKS];
};

// bank_stream_loops_kernel (FR_STREAM_LOOPS): bank_stream_banks_kernel's work -- the bank table also for one bank -- for plans
// whose streamed programs hold feedback loops shorter than a block.  StageProg::pad[0] of a streamed program is its STRIDE
// (streamplan.hpp stream_loop_prepare): 0 = the program runs lane = frame, as in the other kernels; 1..BANK_STREAM_LOOP_MAX_STRIDE
// = a loop program, which the finishing wave runs in three phases on a block of n frames at `head`:
//   1. all lanes, lane = frame: the program's S_INPUTs and S_READs, numbered in program order, go to a load tile
//      [load slot][frame] in LDS, range test applied, four in flight together -- except a read of a ring the program stores
//      itself (S_READ.imm = store slot + 1) whose source frame lies inside the block (lane >= d_lo);
//   2. lanes < stride: lane r walks the frames r, r + stride, ... < n in order, every frame on its own column of the
//      interpreter's registers, operands from the load tile, an own-ring read with f >= d_lo from the store tile
//      [store slot][f - d_lo] -- the same lane wrote it, the stride divides d_lo --, every S_STORE (imm = store slot + 1) into
//      the store tile: no global memory access but the instruction fetch;
//   3. all lanes, lane = frame, live lanes only: the store tile to the rings, the result to its row.
// Before phase 1 the wave copies the program's first BANK_STREAM_LOOP_INSTRS instructions to LDS: phase 2 fetches every
// instruction once per frame, and from global memory each fetch is a dependent trip to L2 (measured: 106 us per block of a
// one-sample comb without the copy, 100 with it; profiles/stream_loops.txt); instructions beyond the copy come from memory.
// The stream's copy of a loop program has no dst_ring (the helper turns it into an S_STORE).  Slots are masked, frame loops
// are bounded by n <= 64.  LDS: the other program kernels' 16 400 bytes + BANK_STREAM_LOOP_LOADS * 256 + BANK_STREAM_LOOP_STORES * 256
// + BANK_STREAM_LOOP_INSTRS * 16 = 36 880.
constexpr uint32_t BANK_STREAM_LOOP_LOADS = 32, BANK_STREAM_LOOP_STORES = 16, BANK_STREAM_LOOP_MAX_STRIDE = 63;   // (powers of two: slots are masked)
constexpr uint32_t BANK_STREAM_LOOP_INSTRS = 512;
// StreamLaunchArgs::max_stride, max_loads, max_stores: the largest stride, load count and store-slot count of the streamed
// programs, as the host prepared them; the launch refuses what the kernel's tiles do not hold.

// bank_stream_general_kernel (FR_STREAM_GENERAL): bank_stream_loops_kernel's work for plans with SCHEDULE BANKS -- voices of any
// partial count and any Sum2 tree, in the general form of launch_gbank (BankArgs::groups / group_off above), and balanced
// voices of 32 or 64 partials as one-item schedules.  Bit `i` of `mask` says that bank i of the StreamBanksArgs table is a
// schedule bank: its Bank::params are the items' pairs, its log2_p and chunk_log2 are not read, and it has ONE workgroup per
// voice (workgroup first_wg + v renders voice first_voice + v) with one chunk, so nothing of it goes through the workspace
// or the tickets.  That workgroup runs the voice's schedule on its 16 waves (kernels.hip stream_render_schedule): an item of
// >= 128 leaves is split over the 16 waves, one of 16 .. 64 leaves over 2 .. 8 waves with a group of 8 each, the sums meet in LDS
// in the tree's own association, one barrier per such item; smaller items and the merges run on wave 0, on an LDS stack.  Every
// barrier's condition comes from the schedule words, which are uniform for the workgroup.  The other banks of the table are
// rendered in chunks as before.  The host validates every schedule before it uploads it (streamplan.hpp stream_schedule_ok).
// LDS: the loops kernel's 36 880 bytes + the stack's 4096 + a second hand-over buffer of 4096 = 45 072.
struct StreamGeneralArgs {
    uint32_t mask;
    struct {
        const uint32_t *groups, *group_off;
    } bank[BANK_STREAM_BANKS];
};

// bank_stream_dyn_kernel (FR_STREAM_DYN): bank_stream_general_kernel's composition -- the same body, one more flag of its form -- for
// plans whose streamed programs delay a voice by a SIGNAL amount: its interpreter also knows S_READ_DYN and S_STEP_DYN, lane =
// frame.  frames = delay_frames(regs[a][lane]) is the reference's cast (shared with pull_kernel and stage_kernel); S_READ_DYN
// yields ring[buf][(frame - frames) & ring_mask] when the cast succeeds and frame >= frames, else 0.0; S_STEP_DYN yields
// bits(imm) under the same condition.  The read is a relaxed agent-scope atomic load like every ring access here: the rule
// admits a bank's ring and (FR_STREAM_TAPS) a ring that an earlier program of the same voice, segment or bus segment stores,
// whose frames of this block the wave itself (a bus program: every voice and its programs) has stored and acknowledged -- the
// interpreter waits for the wave's own stores (s_waitcnt vmcnt(0)) before every program --, so no acquire, release, poll or wait
// is added.  The index is masked: an address is inside the rings whatever the amount.
// A plan without schedule banks is launched with mask == 0 (no schedule table).  The loop phases know no _DYN op: the rule
// refuses one inside a loop program (the sweep forms below, FR_STREAM_SWEEP, have the phase that knows them).  LDS: the general
// kernel's 45 072 bytes.

// bank_stream_hist_kernel (FR_STREAM_HISTORY): bank_stream_dyn_kernel's composition and one more flag, for plans whose streamed
// programs read an INPUT ROW at a delay: S_READ_INPUT (any constant delay, also inside a loop program, where it is one more
// frame-only load of phase 1) and S_READ_INPUT_DYN (lane = frame).  The stream keeps a HISTORY of its n_rows streamed rows,
// hist[row][frame & mask], mask + 1 >= the deepest input read + 64 floats per row: wave 0 of workgroup 0 stores every block's
// live lanes there right after it has republished the rows, under the same acknowledgement, before it stores n_times and seq.
// S_READ_INPUT yields frame >= d_lo ? hist[imm & 7][(frame - d_lo) & mask] : 0.0 (imm: the streamed row, as for S_INPUT);
// S_READ_INPUT_DYN is stream_prog_dyn with the history as its rings.  Every load is a relaxed agent-scope atomic load.  Why no
// wait, acquire or release is added:
//   * frames of the current block (a delay below 64, a signal amount of 0): workgroup 0 had them acknowledged before it stored
//     seq, and a reader loads after it has seen seq -- the hand-over BankStreamInDev::rows has always relied on;
//   * older frames: an earlier block's stores, acknowledged before that block's seq;
//   * block k + 1's stores cannot pass block k's reads: the host rings k + 1 only after k's done tag, the tag follows every
//     voice's ticket, and a ticket follows the acknowledged row stores that depend on those loads;
//   * mask + 1 >= look-back + 64 keeps a block's stores off the frames it reads, and the host zeroes the history before every
//     launch (a launch follows a seek, after which every earlier input reads 0.0), so `frame >= d` is the whole range test.
// Indices are masked: an address is inside the history whatever the amount.  LDS: the general kernel's 45 072 bytes.
struct StreamHistArgs {
    float *hist;               // [n_rows][mask + 1]
    uint64_t mask;
};

// bank_stream_fx_kernel (FR_STREAM_EFFECTS): the resident body for a plan WITHOUT A VOICE -- an echo, a comb or a flanger on a row
// the host feeds in, a gain on a control row -- whose programs the rule has dealt over SEGMENTS (streamplan.hpp): workgroup s is
// ONE WAVE (64 threads: the 16 waves of the other forms exist only to render partials) that runs progs[voice_first[s] ..
// voice_first[s + 1]) of every block, lane = frame, with everything the hist form's interpreter knows -- control rows, loop
// programs, Delays by a signal amount, the history of the streamed rows --, then takes the block's ticket as a finished voice
// does; the last arriver runs the bus segment progs[voice_first[segments] .. voice_first[segments + 1]) and writes the done tag.
// There is no bank, no table, no render, no chunk hand-over and no voice to store: BankArgs gives n_voices = segments and out, and
// its params, rows, ws and tickets are not read.  Row 0 is the time row as ever, S_INPUT(0) the lane's word of it.  Wave 0 of
// workgroup 0 waits on the doorbell, republishes the rows and stores the history exactly as in the hist form; the history exists
// also when no program reads it (64 frames per row).  Why no wait, acquire or release is added:
//   * a read below a block of a ring an EARLIER program stored: the rule put both programs into one segment (the tap behind a
//     loop, a row copy), so it is the same wave's own store, acknowledged (s_waitcnt vmcnt(0)) before the next program's loads --
//     the hand-over the tap behind a voice's loop has always relied on;
//   * a read a block or more back, of any ring and of any row's history: an earlier block's store, acknowledged before that
//     block's ticket, and the host rang this block only after that block's done tag;
//   * the bus segment runs in the wave that drew the block's last ticket: every segment had its stores acknowledged before its
//     ticket, and that wave issues its loads after its own ticket came back -- stream_finish_bus as it stands.
// LDS: the interpreter's registers, the loop tiles and the instruction copy, 32 776 bytes; the waves' sums and the schedule stack
// of the other forms take none here.
//
// bank_stream_store_kernel, bank_stream_store_fx_kernel (FR_STREAM_STORE): the hist form and the fx form with one thing more --
// the stream STORES what it is fed.  Workgroup 0's wave 0, which holds every streamed row of the block in registers and stores
// it to the stream's history, also appends it to the renderer's input store: lane i < n_times of streamed row j goes to
// row[j].data[head + i - row[j].base], the slot's own buffer (engine.cpp InSlot), where fr_fill_buffer, an edited plan's
// look-back rebuild and the next stream find it.  data == null: the slot has no buffer -- a launch-uniform skip.  The store is
// a relaxed agent-scope VECTOR store like the history's, issued with it and acknowledged by the wait's one s_waitcnt vmcnt(0),
// so before n_times and seq: a done tag the host has seen implies that its block's rows are in the store.  Nothing of the
// launch reads those words, so no poll, acquire or release is added.  The host (streamstore.hpp) keeps
// head + n_times - base within the buffer for every slot with a buffer and relaunches before it would not.
struct StreamStoreArgs {
    struct Row {
        float *data;           // the slot's buffer (null: none), data[i] is frame base + i
        uint64_t base;
    } row[BANK_STREAM_ROWS];
};

// bank_stream_sweep_kernel, bank_stream_sweep_fx_kernel, bank_stream_sweep_store_kernel, bank_stream_sweep_store_fx_kernel
// (FR_STREAM_SWEEP): the hist, fx, store and store_fx forms with one flag more (StreamForm::sweep) -- phase 2 of a loop program is
// a uniform loop over SWEEPS, and its interpreter knows the Delays by a signal amount.  StageProg::pad[0] of a loop program is its
// sweep width w, 1..63 (streamplan.hpp stream_sweep_prepare; a loop program of constant stride: its stride): every read of a ring
// the program stores reaches at least w frames back, so the frames [base, base + w) of a block depend only on frames < base.
// Phases 0, 1 and 3 are the loops kernel's (phase 1 knows no _DYN op and skips it); phase 2 is
//   for (base = 0; base < n; base += w)      -- w, n uniform for the wave
//       lane < w, f = base + lane < n: one frame of the interpreter on register column f; then a wave phase
// with the loops kernel's cases and three more:
//   S_READ_DYN        fr = delay_frames(regs[a][f]).  The cast fails or head + f < fr: 0.0.  An own ring (imm = store slot + 1) and
//                     fr <= f: the store tile [slot][(f - fr) & 63] -- a column below `base`, which an earlier iteration of this
//                     wave wrote.  Else stream_prog_dyn's masked relaxed agent-scope load: a frame before the block, any other ring;
//   S_STEP_DYN        stream_prog_dyn;
//   S_READ_INPUT_DYN  stream_prog_dyn on the history of the streamed rows.
// Why no wait, acquire, release, poll or s_barrier is added:
//   * frames of this block: a frame of a sweep reads store-tile columns <= f - w < base, which earlier iterations of this ONE wave
//     wrote -- LDS accesses of a wave complete in program order, the guarantee phase 2 has always relied on, now across lanes;
//   * frames before the block: earlier blocks' ring stores, acknowledged before those blocks' tickets;
//   * bank rings and earlier programs' rings: stored by this wave and waited for (s_waitcnt vmcnt(0)) before the program starts.
// Every index is masked: an amount that violated its proof (fr < w) would read a stale column of the tile, never outside the tile
// or the rings; every loop is bounded by n <= 64.  LDS: the form's underneath (45 072 with voices, 32 776 without).
//
// bank_stream_leaf_kernel, bank_stream_leaf_store_kernel (FR_STREAM_LEAVES): the hist form and the store form with one flag more
// (StreamForm::leaf) -- a LEAF BANK, a bank of compiled voices (stage.hpp BankLaunch::jit: leaves of one arbitrary expression
// shape, which fr_fill_buffer renders with a hipRTC-generated kernel), is rendered by a LEAF INTERPRETER.  Bit `i` of
// StreamLeafArgs::mask says that bank i of the StreamBanksArgs table is a leaf bank: its Bank::params is the bank's uploaded
// parameter table [voice][1 << log2_p][k] floats, k = StreamLeafArgs::bank[i].k, and it is chunked over workgroups exactly as a
// template bank (16 waves x groups of 8, one workgroup per (voice, chunk)).  Its leaf is a program (leafprog.hpp): n_instr
// instructions `dst = a op b` over BANK_STREAM_LEAF_REGS registers, an operand a register, a parameter column, a literal or a
// streamed row at the lane's frame (LEAF_IN's operand is the ROW, rewritten by the engine as S_INPUT's is).
// kernels.hip stream_render_leaves: lane = frame, a wave walks its 1/16 of the chunk's partials; per partial it runs the program
// on its own LDS register columns regs[wave][register][lane] -- instruction words and parameters are uniform and come through the
// scalar cache --, every op through prim_binop, separately rounded; the leaves are summed literally in the graph's association
// (a group of 8 as ((l0+l1)+(l2+l3))+((l4+l5)+(l6+l7)), the binary-counter carry chain over the wave's groups, the 16 wave sums
// in tree order through LDS, the chunk sums through stream_hand_over).  Every add is performed, so a zero has the graph's sign
// and there is no repair pass.  The block's streamed rows are staged once per block in LDS (wave j loads row j, one barrier, under
// the workgroup-uniform condition that its bank is a leaf bank).  No acquire, release, poll or wait is added: the rows were
// republished before the workgroup saw the block's seq, as the time row always was.
// LDS: the form underneath (45 072) + the register file 16 x 8 x 256 = 32 768 + the staged rows 8 x 256 = 2 048: 79 888.
constexpr uint32_t BANK_STREAM_LEAF_INSTRS = 32, BANK_STREAM_LEAF_REGS = 8;
struct StreamLeafArgs {
    uint32_t mask;
    struct Bank {
        const uint4 *instrs;       // [n_instr] {op | dst << 8 | ka << 16 | kb << 24, a, b, 0} (leafprog.hpp LeafInstr)
        uint32_t n_instr, k;       // instructions (0: the leaf is its result operand), floats per partial of the parameter table
        uint32_t result_kind, result;   // the leaf's value as an operand
    } bank[BANK_STREAM_BANKS];
};

//
// bank_stream_track_kernel, bank_stream_track_store_kernel (FR_STREAM_TRACKS): the two leaf forms with one flag more
// (StreamForm::tracks) -- a leaf bank's leaf may read TRACK rows (leafshape.hpp LEAF_TRACK: per-partial frequency and amplitude
// rows of the block's dense input matrix, fr_stream_block_dense).  The host copies the block's track rows into a STAGING matrix
// of mapped pinned memory, staging[(slot - first_slot) * 64 + frame], before it writes the doorbell, and puts the block's slot
// limit and row count into BankStreamInCtl::tracks.  A track operand (leafprog.hpp LEAF_TRK, after the engine's upload: `v` = its
// place q in StreamTrackArgs::Bank::cols) is, for lane = frame,
//     slot < limit && slot - first_slot < rows && lane < T ? staging[(slot - first_slot) * 64 + lane] : +0.0
// where slot is the bits of parameter column cols[q] of the partial's row (a literal column: cols[q] itself) -- jit_track's
// value (leafjit.cpp) with the dense call's limit.  The loads are relaxed SYSTEM-scope atomic loads, issued only after the
// workgroup has passed stream_next_block for this block (the host wrote the matrix, then a release fence, then the doorbell).
// Each is a trip across PCIe, so a wave has the rows of partial j + 1 in flight while it interprets partial j: the values wait in
// registers and are PARKED, at the top of the next iteration, in the wave's own columns trk[wave][j & 1][q][lane] of LDS, where
// the interpreter's uniform operand switch reads them.  Only the owning wave touches its columns (a wave's LDS accesses complete
// in program order): no barrier, acquire or poll is added.  One staging buffer suffices: the host writes the next block's matrix
// only after this block's done tag, which follows every voice's ticket, which follows every wave's last track read.
// LDS: the leaf form's 79 888 + 16 x 2 x 4 x 256 = 32 768: 112 656.
constexpr uint32_t BANK_STREAM_LEAF_TRACKS = 4;
constexpr uint32_t BANK_STREAM_TRACK_ROWS = 65536;   // the staging's largest row count: 256 workgroups x 128 partials x 2 rows, 16 MiB
struct StreamTrackArgs {
    const float *staging;          // [rows][64], mapped pinned host memory as the device addresses it
    uint32_t first_slot, rows;     // the slot of staging row 0 (fr_set_track_inputs), the rows the allocation holds
    struct Bank {
        uint32_t n, literal;       // track operands of the bank's leaf (<= BANK_STREAM_LEAF_TRACKS); bit q: cols[q] is the slot itself
        uint32_t cols[BANK_STREAM_LEAF_TRACKS];   // else the parameter column (< StreamLeafArgs::Bank::k) that holds the slot's bits
    } bank[BANK_STREAM_BANKS];
};

// The twenty resident kernels (streamplan.hpp stream_launch chooses; `none`: no resident launch yet) and their one launch entry.
// plain, prog and bus have the one-row doorbell (BankStreamCtl / BankStreamDev), the others the doorbell of rows (BankStreamIn*).
// (hist is dyn + 2, fx is hist + 2, store is fx + 2, store_fx is store + 2, and the four sweep forms go on by 2: the values in
// between stay unnamed and refused, as the tests of the launch check have always required)
enum class StreamKernel : uint32_t {
    none, plain, prog, bus, in, banks, loops, general, dyn, hist = dyn + 2, fx = hist + 2, store = fx + 2, store_fx = store + 2,
    sweep = store_fx + 2, sweep_fx = sweep + 2, sweep_store = sweep_fx + 2, sweep_store_fx = sweep_store + 2,
    leaf = sweep_store_fx + 4, leaf_store = leaf + 2,   // (the value after the sweep forms stays unnamed as well)
    track = leaf_store + 2, track_store = track + 2
};
constexpr bool stream_kernel_named(StreamKernel k) {
    return k != StreamKernel::none && (k <= StreamKernel::dyn || k == StreamKernel::hist || k == StreamKernel::fx || k == StreamKernel::store || k == StreamKernel::store_fx ||
                                       k == StreamKernel::sweep || k == StreamKernel::sweep_fx || k == StreamKernel::sweep_store || k == StreamKernel::sweep_store_fx ||
                                       k == StreamKernel::leaf || k == StreamKernel::leaf_store || k == StreamKernel::track || k == StreamKernel::track_store);
}
// A kernel's form: what it has on top of bank_stream_kernel.  The nine kernels with voices are a cascade -- each is the one
// before it and one thing more --, so the enum's order is their form; fx, which has no voice, is written out.  kernels.hip's one
// resident body is instantiated by it, stream_launch_check below reads it.
struct StreamForm {
    bool progs;      // runs the voices' programs (StreamProgArgs) and advances `head`
    bool bus;        // ... and the bus segment in the block's last arriver
    bool rows;       // the doorbell of n_rows rows, S_INPUT by row; else the one-row doorbell
    bool table;      // a workgroup finds its bank in the table (StreamBanksArgs); else the one bank of BankArgs
    bool loops;      // loop programs: the load and store tiles and the instruction copy
    bool schedule;   // schedule banks (StreamGeneralArgs)
    bool dyn;        // the interpreter knows the Delays by a signal amount; a plan need not have a schedule bank
    bool hist;       // the history of the streamed rows (StreamHistArgs): delayed reads of input rows
    bool voiceless;  // no bank at all: a workgroup is one wave that runs a segment of programs (fx, store_fx)
    bool store = false;   // workgroup 0 also appends the streamed rows to the input store (StreamStoreArgs): store, store_fx
    bool sweep = false;   // a loop program's phase 2 walks sweeps and knows the Delays by a signal amount: the four sweep forms
    bool leaf = false;    // leaf banks (StreamLeafArgs): compiled voices rendered by the leaf interpreter: leaf, leaf_store, track, track_store
    bool tracks = false;  // ... whose leaves may read track rows of the block's staged matrix (StreamTrackArgs): track, track_store
};
constexpr StreamForm stream_form(StreamKernel k) {
    // the track forms: the leaf forms and the flag
    if (k == StreamKernel::track) return {true, true, true, true, true, true, true, true, false, false, false, true, true};
    if (k == StreamKernel::track_store) return {true, true, true, true, true, true, true, true, false, true, false, true, true};
    // the leaf forms: the hist form and the store form, and the flag
    if (k == StreamKernel::leaf) return {true, true, true, true, true, true, true, true, false, false, false, true};
    if (k == StreamKernel::leaf_store) return {true, true, true, true, true, true, true, true, false, true, false, true};
    // the sweep forms: the form underneath and the flag
    if (k == StreamKernel::sweep) return {true, true, true, true, true, true, true, true, false, false, true};          // hist
    if (k == StreamKernel::sweep_fx) return {true, true, true, false, true, false, true, true, true, false, true};      // fx
    if (k == StreamKernel::sweep_store) return {true, true, true, true, true, true, true, true, false, true, true};     // store
    if (k == StreamKernel::sweep_store_fx) return {true, true, true, false, true, false, true, true, true, true, true}; // store_fx
    if (k == StreamKernel::fx)   // progs, bus, rows, loops, dyn and hist; no table, no schedule
        return {true, true, true, false, true, false, true, true, true};
    if (k == StreamKernel::store_fx) return {true, true, true, false, true, false, true, true, true, true};   // fx and the store
    if (k == StreamKernel::store) return {true, true, true, true, true, true, true, true, false, true};       // hist and the store
    return {k >= StreamKernel::prog,  k >= StreamKernel::bus,     k >= StreamKernel::in,  k >= StreamKernel::banks,
            k >= StreamKernel::loops, k >= StreamKernel::general, k >= StreamKernel::dyn, k == StreamKernel::hist, false};
}
// Everything a resident launch may need; stream_launch_check reads and checks what the kernel takes.
struct StreamLaunchArgs {
    BankArgs a;
    StreamProgArgs p;
    StreamBanksArgs t;
    StreamGeneralArgs g;
    StreamHistArgs h;                           // (read for the forms with a history)
    StreamStoreArgs s;                          // (read for the store forms)
    StreamLeafArgs l;                           // (read for the leaf forms)
    StreamTrackArgs tr = {};                    // (read for the track forms)
    uint32_t n_rows, max_stride, max_loads, max_stores;
    void *ctl_dev, *dev;                        // the control block as the device addresses it and the device block, of the kernel's doorbell form
    uint32_t idle_ms;                           // 0 = BANK_STREAM_IDLE_MS
};
hipError_t launch_bank_stream(StreamKernel k, const StreamLaunchArgs &x, hipStream_t s);

// What every resident launch checks of a balanced bank's shape, and of the programs' arguments.  (chunk_log2 >= 7: each of
// the 16 waves gets a whole group of 8 partials.)
inline bool stream_bank_ok(uint32_t log2_p, uint32_t chunk_log2, uint32_t n_voices, const float *ws, const uint32_t *tickets) {
    if (chunk_log2 < 7 || chunk_log2 > 13 || chunk_log2 > log2_p || log2_p - chunk_log2 > 8) return false;
    if (((uint64_t)n_voices << (log2_p - chunk_log2)) > BANK_STREAM_WGS || n_voices == 0) return false;   // all workgroups must be resident
    return chunk_log2 == log2_p || (ws && tickets);
}
inline bool stream_progs_ok(const StreamProgArgs &p, bool to_ring) {
    if (!p.voice_first || (p.ring_mask & (p.ring_mask + 1)) != 0) return false;
    return !(p.n_rings && (!p.rings || p.ring_mask + 1 < 64u)) && !(to_ring && !p.n_rings);
}
// The bank table: every bank as the one-bank kernels' bank; the banks' workgroups and voices follow one another without a
// gap.  `schedule_mask`: the schedule banks (StreamGeneralArgs::mask), one workgroup per voice whatever their log2_p and
// chunk_log2 say.  Returns the launch's workgroups (0: refused) and whether a bank feeds rings.
inline uint32_t stream_table_ok(const StreamBanksArgs &t, const BankArgs &a, uint32_t schedule_mask, bool &to_ring) {
    if (t.n_banks == 0 || t.n_banks > BANK_STREAM_BANKS || (schedule_mask >> t.n_banks) != 0) return 0;
    uint64_t wgs = 0, voices = 0;
    to_ring = false;
    for (uint32_t i = 0; i < t.n_banks; ++i) {
        const StreamBanksArgs::Bank &b = t.bank[i];
        const bool schedule = (schedule_mask >> i) & 1u;
        if (schedule ? b.n_voices == 0 : !stream_bank_ok(b.log2_p, b.chunk_log2, b.n_voices, a.ws, a.tickets)) return 0;
        if (!b.params || !b.rows || b.first_wg != wgs || b.first_voice != voices) return 0;
        wgs += schedule ? (uint64_t)b.n_voices : (uint64_t)b.n_voices << (b.log2_p - b.chunk_log2);
        voices += b.n_voices;
        if (wgs > BANK_STREAM_WGS) return 0;   // all workgroups must be resident
        to_ring = to_ring || b.to_ring != 0;
    }
    return voices == a.n_voices ? (uint32_t)wgs : 0;
}

// What launch_bank_stream checks before it launches kernel `k`, by the kernel's form: plain host logic, so it is tested without
// a device (tests/cpp/streamcheck_tests.cpp).  Returns the workgroups to launch -- exactly those that render: a small patch
// leaves the other CUs to whatever else wants the device --, 0: refused.
inline uint32_t stream_launch_check(StreamKernel k, const StreamLaunchArgs &x) {
    if (!stream_kernel_named(k)) return 0;
    const StreamForm f = stream_form(k);
    const BankArgs &a = x.a;
    if (a.leaf_variant != 1 || !a.out || !x.ctl_dev || !x.dev) return 0;
    if (f.rows && (x.n_rows == 0 || x.n_rows > BANK_STREAM_ROWS)) return 0;
    if (f.hist && (!x.h.hist || (x.h.mask & (x.h.mask + 1)) != 0 || x.h.mask + 1 < 64u)) return 0;   // a ring of 2^n >= 64 frames per row
    // the tiles' limits concern loop programs; the general form takes a plan without one (max_stride == 0)
    if (f.loops && (x.max_stride > BANK_STREAM_LOOP_MAX_STRIDE || x.max_loads > BANK_STREAM_LOOP_LOADS || x.max_stores > BANK_STREAM_LOOP_STORES)) return 0;
    if ((f.schedule || f.voiceless ? x.max_stride != 0 : f.loops) && !x.p.n_rings) return 0;   // a loop lives in a ring
    uint32_t wgs = 0;
    bool to_ring = f.progs && x.p.bank_to_ring != 0;
    if (f.voiceless) {
        // no bank: n_voices is the segment count, a workgroup of one wave each; params, rows, ws, tickets and the tables are not read
        if (a.n_voices == 0 || a.n_voices > BANK_STREAM_WGS) return 0;   // all workgroups must be resident
        wgs = a.n_voices;
        to_ring = false;
    } else if (f.table) {
        const uint32_t mask = f.schedule ? x.g.mask : 0u;
        if (f.schedule && !f.dyn && mask == 0) return 0;   // (only dyn takes a plan without a schedule bank)
        wgs = stream_table_ok(x.t, a, mask, to_ring);
        if (!wgs) return 0;
        if (f.leaf) {
            // a leaf form is launched for a plan with a leaf bank; a leaf bank is chunked (stream_table_ok has checked it as a
            // template bank's shape), never a schedule bank, and its program is within the interpreter's limits
            const uint32_t leaves = x.l.mask;
            if (leaves == 0 || (leaves >> x.t.n_banks) != 0 || (leaves & mask) != 0) return 0;
            for (uint32_t i = 0; i < x.t.n_banks; ++i) {
                if (!((leaves >> i) & 1u)) continue;
                const StreamLeafArgs::Bank &lb = x.l.bank[i];
                if (lb.n_instr > BANK_STREAM_LEAF_INSTRS || (lb.n_instr && !lb.instrs) || lb.k == 0 || lb.result_kind > (f.tracks ? 4u : 3u)) return 0;
                if (lb.result_kind == 0u && (lb.n_instr == 0 || lb.result >= BANK_STREAM_LEAF_REGS)) return 0;   // a register nobody wrote
                if (lb.result_kind == 1u && lb.result >= lb.k) return 0;
                if (lb.result_kind == 3u && lb.result >= x.n_rows) return 0;
                if (f.tracks) {
                    // a track form: the bank's track operands number at most BANK_STREAM_LEAF_TRACKS, each slot column is one of the
                    // table's k, and a leaf that is a bare track names one of them
                    const StreamTrackArgs::Bank &tb = x.tr.bank[i];
                    if (tb.n > BANK_STREAM_LEAF_TRACKS || (tb.literal >> tb.n) != 0) return 0;
                    for (uint32_t q = 0; q < tb.n; ++q)
                        if (!((tb.literal >> q) & 1u) && tb.cols[q] >= lb.k) return 0;
                    if (lb.result_kind == 4u && lb.result >= tb.n) return 0;
                }
            }
            // ... and the staging matrix with its row count (a plan whose slots the staging cannot hold is the rule's to refuse)
            if (f.tracks && (!x.tr.staging || x.tr.rows == 0 || x.tr.rows > BANK_STREAM_TRACK_ROWS || x.tr.first_slot > UINT32_MAX - x.tr.rows)) return 0;
        }
        for (uint32_t i = 0; i < x.t.n_banks; ++i)
            if (((mask >> i) & 1u) && (!x.g.bank[i].groups || !x.g.bank[i].group_off)) return 0;
    } else {
        if (!stream_bank_ok(a.log2_p, a.chunk_log2, a.n_voices, a.ws, a.tickets) || !a.rows) return 0;
        wgs = a.n_voices << (a.log2_p - a.chunk_log2);
    }
    return !f.progs || stream_progs_ok(x.p, to_ring) ? wgs : 0;
}

// The host's side of a doorbell by its form: all its words (the stop goes to every one), the done tag, the two blocks' sizes.
static_assert(offsetof(BankStreamCtl, row) == offsetof(BankStreamInCtl, rows), "a one-row doorbell is the first row of a doorbell of rows");
static_assert(offsetof(BankStreamCtl, done) == sizeof(BankStreamCtl::row) && offsetof(BankStreamCtl, alive) == offsetof(BankStreamCtl, done) + 4 &&
              offsetof(BankStreamInCtl, done) == sizeof(BankStreamInCtl::rows) && offsetof(BankStreamInCtl, alive) == offsetof(BankStreamInCtl, done) + 4, "done and alive follow the rows");
struct StreamDoorbell {
    unsigned long long *words;
    size_t n_words;
    uint32_t *done;
    size_t ctl_bytes, dev_bytes;
};
inline StreamDoorbell stream_doorbell(void *ctl, bool rows) {
    if (rows) {
        BankStreamInCtl *c = static_cast<BankStreamInCtl *>(ctl);
        return {c ? c->rows[0] : nullptr, (size_t)BANK_STREAM_ROWS * 64, c ? &c->done : nullptr, sizeof(BankStreamInCtl), sizeof(BankStreamInDev)};
    }
    BankStreamCtl *c = static_cast<BankStreamCtl *>(ctl);
    return {c ? c->row : nullptr, 64, c ? &c->done : nullptr, sizeof(BankStreamCtl), sizeof(BankStreamDev)};
}

// One step of the partial-block exchange (friendship_render.h FR_SHARD_PARTIALS): row i, window frame t:
//   v = lo[i][t] + hi[i][t]         the Sum2 node one level up: left sub-tree + right sub-tree, one f32 add
// stored to dst_ws[i][t] (steps before the last; may alias lo or hi), or -- the last step, dst_ws == null -- where the
// unsharded plan puts the voice: dst[i] bit 31 set: ring dst[i] & 0x7FFFFFFF at absolute frame ring_t0 + t; else
// output row dst[i], frames t >= out_skip only (the look-back part of a window is not output).
struct ShardCombineArgs {
    const float *lo;
    const float *hi;
    float *dst_ws;
    const uint32_t *dst;
    float *out;
    uint64_t out_stride;
    uint64_t out_skip;
    float *rings;
    uint64_t ring_mask;
    uint64_t ring_t0;
    uint32_t n_rows;
    uint64_t len;
};
hipError_t launch_shard_combine(const ShardCombineArgs &a, hipStream_t s);

// A voice rendered as 2^log2_c consecutive pieces of its leaves (a short call of few voices would not fill the chip
// otherwise): ws holds the pieces' sums as rows [(voice << log2_c) | piece][n_times]; this adds them up the way the voice's
// Sum2 tree does above the pieces -- adjacent pairs, level by level -- and stores the voice at out[rows[voice]].  log2_c <= 6.
struct ChunkCombineArgs {
    const float *ws;
    float *out;
    const uint32_t *rows;
    uint64_t out_stride;
    uint64_t n_times;
    uint32_t n_voices;
    uint32_t log2_c;
};
hipError_t launch_chunk_combine(const ChunkCombineArgs &a, hipStream_t s);

// Fills dst[0..n) with *src_last (or 0 when src_last is null): last-value padding of a short input
// row (reference.rs:72-73) for the device-resident entry point.
hipError_t launch_pad(float *dst, uint64_t n, const float *src_last, hipStream_t s);

// Value range of input rows (FR_DELAY_OBSERVED, stage.hpp ObservedInputs): block (b, r) reduces the elements
// b*256 + tid, stepping by blocks*256, of row r into out[r * blocks + b] -- min and max of the finite values, and flags for
// NaN, +inf and -inf.  The host merges a row's `blocks` partial results; `out` is mapped pinned memory.
constexpr uint32_t RANGE_NAN = 1u, RANGE_POS_INF = 2u, RANGE_NEG_INF = 4u;
constexpr uint32_t RANGE_MAX_ROWS = 32, RANGE_MAX_BLOCKS = 64, RANGE_THREADS = 256;
struct RangePart {
    float lo, hi;        // +inf / -inf: no finite value
    uint32_t flags, pad;
};
struct RangeArgs {
    const float *row[RANGE_MAX_ROWS];
    uint64_t len[RANGE_MAX_ROWS];
    uint32_t n_rows, blocks;
    RangePart *out;
};
hipError_t launch_input_range(const RangeArgs &a, hipStream_t s);

// Track history (FR_TRACK_HISTORY): the renderer keeps the last frames of every track row (fr_set_track_inputs) in a ring of
// mask + 1 floats per row (a power of two), frame f of row r at tail[r * (mask + 1) + (f & mask)].  A call appends the last
// `count` columns of its rows: lanes over consecutive frames of a row, a wave per row, 16-byte loads and stores where the
// source and the destination are equally aligned; rows [src_rows, rows) -- not supplied -- are appended as +0.0.
struct TrackTailArgs {
    float *tail;
    const float *src;          // the call's row of the first track slot (rows src_stride floats apart); null: none supplied
    uint64_t src_stride;
    uint32_t src_rows, rows;
    uint64_t mask;
    uint64_t first;            // absolute frame of the first appended column
    uint64_t col0;             // ... and its column in the call's rows
    uint64_t count;            // columns appended per row (at most mask + 1)
};
hipError_t launch_track_tail(const TrackTailArgs &a, hipStream_t s);

// A track slot read further back than the call's own frames (programs, the pull interpreter, template voices): its window
// [idx - back, idx + n) gathered into dst[i] -- the `back` frames before idx from the tail ring (null: +0.0), the call's
// frames from its row (null: not supplied, +0.0).  Row i of the launch is blockIdx.y.
constexpr uint32_t TRACK_WINDOW_MAX_ROWS = 32;
struct TrackWindowArgs {
    float *dst[TRACK_WINDOW_MAX_ROWS];
    const float *tail[TRACK_WINDOW_MAX_ROWS];
    const float *call[TRACK_WINDOW_MAX_ROWS];
    uint32_t n_rows;
    uint64_t mask, idx, back, n;
};
hipError_t launch_track_window(const TrackWindowArgs &a, hipStream_t s);

// Kept delay lines (FR_RING_KEEP): after a re-plan the rings whose contents are still right go from the old allocation
// (rows of src_mask + 1 floats, frame f at f & src_mask) to the row and capacity the new plan gives them in a second
// allocation: a streaming gather over a device array of descriptors.  A wave takes one segment of a descriptor's frames, cut
// at multiples of RING_MOVE_SEG: capacities are powers of two of at least that, so a segment is contiguous on both sides
// (no ring wraps inside one) and source and destination are equally aligned -- 16-byte accesses with element-wise heads
// and tails.  `host_desc`: the same descriptors in host memory; the launch bounds every one of them before it starts.
constexpr uint64_t RING_MOVE_SEG = 1024;
struct RingMoveDesc {
    uint32_t src_row, dst_row;
    uint64_t first, count;     // absolute frames [first, first + count)
};
struct RingMoveArgs {
    const float *src;
    float *dst;
    uint64_t src_mask, dst_mask;
    uint32_t src_rows, dst_rows;       // rows of the two allocations
    const RingMoveDesc *desc;          // as the device addresses them
    const RingMoveDesc *host_desc;
    uint32_t n_desc;
};
inline bool ring_move_in_bounds(const RingMoveArgs &a) {
    if (!a.src || !a.dst || !a.desc || !a.host_desc) return false;
    const uint64_t sc = a.src_mask + 1, dc = a.dst_mask + 1;
    if ((sc & a.src_mask) != 0 || (dc & a.dst_mask) != 0 || sc < RING_MOVE_SEG || dc < RING_MOVE_SEG) return false;
    for (uint32_t i = 0; i < a.n_desc; ++i) {
        const RingMoveDesc &d = a.host_desc[i];
        if (d.src_row >= a.src_rows || d.dst_row >= a.dst_rows || d.count > sc || d.count > dc || d.first + d.count < d.first) return false;
    }
    return true;
}
hipError_t launch_ring_move(const RingMoveArgs &a, hipStream_t s);

}  // namespace fr
