// engine.cpp -- the HIP render engine behind include/friendship_render.h.
//
// State contract (reference src/render/reference.rs:21-29): mirrored graph + per-slot input history +
// `head`.  Everything else held here (lowered graph, device tables, bank parameters) is a cache of
// that state, rebuilt when the mirror's version or the number of rendered slots changes.
//
// There is no CPU evaluation path in this file: if no gfx950 device is usable, creating a renderer
// fails with FR_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/friendship_render_ext.h"
#include "bankplan.hpp"
#include "callplan.hpp"
#include "comm.hpp"
#include "graph.hpp"
#include "jit.hpp"
#include "kernels.hpp"
#include "match.hpp"
#include "stage.hpp"
#include "streamplan.hpp"
#include "streamrows.hpp"
#include "streamstore.hpp"

namespace fr {

#define HIP_CHECK(expr)                                                                               \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess)                                                                         \
            throw Error(_e == hipErrorOutOfMemory ? FR_ERR_OUT_OF_MEMORY : FR_ERR_DEVICE,             \
                        std::string(#expr) + ": " + hipGetErrorString(_e));                           \
    } while (0)

// Device allocation owned by the engine.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    void ensure(size_t n) {   // contents are NOT preserved
        if (n <= bytes) return;
        release();
        size_t want = std::max(n, (size_t)256);
        HIP_CHECK(hipMalloc(&p, want));
        bytes = want;
    }
    template <class T> T *as() const { return (T *)p; }
};

// Page-locked host staging memory (DMA without the runtime's own bounce copies; async copies stay async).
struct PinnedBuf {
    void *p = nullptr;
    void *dev = nullptr;     // the same memory as the GPU addresses it (mapped: kernels read and write it over PCIe)
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    void ensure(size_t n) {
        if (n <= bytes) return;
        if (p) (void)hipHostFree(p);
        p = dev = nullptr;
        bytes = 0;
        size_t want = std::max(n, (size_t)4096);
        HIP_CHECK(hipHostMalloc(&p, want, hipHostMallocMapped));
        HIP_CHECK(hipHostGetDevicePointer(&dev, p, 0));
        bytes = want;
    }
    template <class T> T *as() const { return (T *)p; }
    template <class T> T *as_dev() const { return (T *)dev; }
};

// One external input slot's history on the device (reference.rs:25 `inputs[slot]`).
// (its books -- fed, base, len, cap -- are streamstore.hpp StoreSlot, which the store's host rules read)
struct InSlot : StoreSlot {
    DevBuf buf;
};

struct BankStage {
    BankLaunch grp;          // rows/params kept on the host for the plan description
    DevBuf d_params, d_rows, d_groups, d_group_off;
    std::shared_ptr<JitKernel> jit;   // grp.jit: the hipRTC specialisation
};

struct Plan {
    bool valid = false;
    uint64_t version = 0;
    uint64_t shard_epoch = 0;            // fr_set_shard generation the plan was made for
    bool jit_pending = false;            // planned without a kernel that hipRTC is still compiling in the background:
    uint64_t jit_epoch = 0;              // stale as soon as the cache's epoch moves on
    uint32_t n_slots = 0;
    uint32_t max_depth = 0;              // of the lowered graph (pull stack sizing)
    std::vector<BankStage> banks;
    StagedPlan sp;                       // programs / levels / rings (banks moved into `banks`)
    DevBuf d_instrs, d_progs;
    std::shared_ptr<JitKernel> stage_jit;   // compiled form of the programs (null: interpreted by stage_kernel)
    DevBuf d_jprogs, d_ptab;
    uint32_t stage_shapes = 0;
    StageJitPlan stage_jit_form;         // stage_jit's generated form (deep ... blk; its source and rows are not kept)
    bool stage_valid = false;            // rings hold [stage_end - lmax, stage_end) of the current graph + history
    uint64_t stage_end = 0;
    std::vector<uint32_t> pull_rows;     // output rows evaluated by the pull interpreter
    DevBuf d_split_dst;                  // partial-block sharding: destination (row, or ring | 1 << 31) per exchange workspace row
    DevBuf d_nodes, d_roots;             // pull: nodes (input slots remapped dense), roots per pull row
    std::vector<uint32_t> input_slots;   // dense input index -> external slot
    const FlatGraph *graph = nullptr;    // the lowered graph the plan was made from (Lowering::update: stable)
    bool observed_stale = false;         // FR_DELAY_OBSERVED: stored rows widened an input range past a planned look-back
    LoopTile loop_tile;                  // FR_LOOP_TILES (callplan.hpp loop_tile): frames per tile of the strided launches, 0: not tiled
    LoopSweep loop_sweep;                // FR_LOOP_DYN (callplan.hpp loop_sweep): the launch form of a sweep plan's fused programs
    std::string json;
};

// One bank launch of the last call, as fr_plan_json's "bank_launches" shows it.
struct BankLaunchNote {
    BankPlan launch;
    uint32_t voices, partials;
    uint64_t frames;
    uint32_t log2_p, leaf_variant;       // (with row_flags: what bankplan.hpp bank_variant reads besides the plan)
    bool row_flags;
    const char *form;                    // FR_RING_KEEP: "call", "repair" (rebuilt rings up to idx) or "replay" (a loop from 0)
};

// One stage-program launch of the last call, as fr_plan_json's "stage_launches" shows it.
struct StageLaunchNote {
    const char *form;                    // levels, fused, strided, feedback, copy, replay, repair
    bool jit;                            // jit_stage (else stage_kernel)
    uint32_t programs;
    uint64_t frames, stride;
    bool carry, carry_only, table;       // use_carry (stage_kernel's LDS carry), carry_only, input table in device memory
    uint32_t grid_parts;                 // launches of at most 65535 programs (grid.y) it was cut into
    bool tile = false;                   // FR_LOOP_TILES: stage_tile_kernel / jit_stage_tile
    uint32_t sweep = 0;                  // FR_LOOP_DYN: 1 = stage_sweep_kernel (frames = the window, stride = frames per sweep),
                                         // 2 = one window of the windows form (stage_kernel, stride 0)
};

// fr_plan_json "stage_jit_form": the #defines plan_stage_jit wrote for the plan's compiled programs, null when interpreted.
// `with_tile` (FR_LOOP_TILES was given): and "tile", the frames per tile its jit_stage_tile was generated for (0: it has none).
static std::string stage_jit_form_json(const Plan &p, bool with_tile) {
    if (!p.stage_jit) return "null";
    const StageJitPlan &f = p.stage_jit_form;
    return std::string("{\"deep\":") + (f.deep ? "true" : "false") + ",\"maxp\":" + std::to_string(f.maxp) + ",\"maxld\":" + std::to_string(f.maxld) +
           ",\"maxst\":" + std::to_string(f.maxst) + ",\"defer\":" + (f.defer ? "true" : "false") + ",\"blk\":" + std::to_string(f.blk) +
           ",\"shapes\":" + std::to_string(p.stage_shapes) + (with_tile ? ",\"tile\":" + std::to_string(f.tile) : std::string()) + "}";
}

// fr_plan_json "stage_hoisted_max": the most loads any program issues back to back before its other instructions (StageProg
// n_loads; 0 where a program has more than STAGE_MAX_HOISTED loads and constants: each is then issued where it is used).
static uint32_t stage_hoisted_max(const StagedPlan &sp) {
    uint32_t m = 0;
    for (const StageProg &pg : sp.progs) m = std::max(m, pg.n_loads);
    return m;
}

// A stage launch as one key (fr_plan_json "stage_launches" "variant"): the kernel -- jit_stage with its generated form
// [plain|deep, P (MAXP > 0), defer, B<BLK>] -- then the launch form and the paths the launch's arguments select:
// +carry / +carry_only (stage_kernel: use_carry, the LDS carry; jit_stage keeps it in registers whenever it strides),
// +table (more than STAGE_INLINE_INPUTS input slots: the table in device memory), +grid<N> (cut into N launches of at most
// 65535 programs).  tests/stage_variants.py has a GPU case for each key the rule produces.  A tiled launch (FR_LOOP_TILES) is
// jit_stage[tile] / jit_stage[tile,P] -- jit_stage_tile has no block and defers every store -- or stage_kernel, and carries +tile
// after the carry flag (tests/loop_tile_cases.py).
static std::string stage_variant(const StageLaunchNote &n, const Plan &p) {
    std::string k = "stage_kernel";
    // (FR_LOOP_DYN: stage_sweep_kernel/feedback+sweep, stage_sweep_kernel/replay+sweep; the windows form: stage_kernel/windows)
    if (n.sweep == 1) k = "stage_sweep_kernel";
    else if (n.jit && n.tile) k = std::string("jit_stage[tile") + (p.stage_jit_form.maxp ? ",P" : "") + "]";
    else if (n.jit) {
        const StageJitPlan &f = p.stage_jit_form;
        k = std::string("jit_stage[") + (f.deep ? "deep" : "plain") + (f.maxp ? ",P" : "") + (f.defer ? ",defer" : "") + ",B" + std::to_string(f.blk) + "]";
    }
    k += std::string("/") + (n.sweep == 2 ? "windows" : n.form);
    if (n.sweep == 1) k += "+sweep";
    if (n.carry_only) k += "+carry_only";
    else if (n.carry) k += "+carry";
    if (n.tile) k += "+tile";
    if (n.table) k += "+table";
    if (n.grid_parts > 1) k += "+grid" + std::to_string(n.grid_parts);
    return k;
}

constexpr size_t N_OPTIONS = 46;        // per-renderer options (friendship_render_ext.h; the table below fr_renderer)

struct TimerClass {
    double ms = 0;
    uint64_t launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// A host-loop definition of the range launch for builds without kernels.hip (the host-logic simulator, whose "device"
// memory is host memory); the HIP library's kernels.hip defines the real one, which the linker takes instead of this.
__attribute__((weak)) hipError_t launch_input_range(const RangeArgs &a, hipStream_t) {
    for (uint32_t r = 0; r < a.n_rows; ++r)
        for (uint32_t b = 0; b < a.blocks; ++b) {
            RangePart o{HUGE_VALF, -HUGE_VALF, 0, 0};
            for (uint64_t i = (uint64_t)b * RANGE_THREADS; i < a.len[r]; i += (uint64_t)a.blocks * RANGE_THREADS)
                for (uint64_t j = i; j < std::min<uint64_t>(i + RANGE_THREADS, a.len[r]); ++j) {
                    const float v = a.row[r][j];
                    if (v != v) o.flags |= RANGE_NAN;
                    else if (v == HUGE_VALF) o.flags |= RANGE_POS_INF;
                    else if (v == -HUGE_VALF) o.flags |= RANGE_NEG_INF;
                    else { o.lo = std::min(o.lo, v); o.hi = std::max(o.hi, v); }
                }
            a.out[(size_t)r * a.blocks + b] = o;
        }
    return hipSuccess;
}

// The sweep launch (FR_LOOP_DYN, kernels.hpp launch_stage_sweep) as a host loop for the simulator, whose launch_stage it calls a
// sweep at a time: sweeps in order, and inside one the order that launch_stage takes for the threads of any launch -- programs
// last to first, frames last to first --, the least favourable one the kernel's threads could take.
__attribute__((weak)) hipError_t launch_stage_sweep(const StageArgs &a, hipStream_t s) {
    if (a.n_progs == 0 || a.w_len == 0) return hipSuccess;
    if (a.n_progs > 65535u || a.sweep == 0 || a.sweep > STAGE_SWEEP_MAX || a.stride != 0 || a.tile != 0 || a.use_carry != 0) return hipErrorInvalidValue;
    StageArgs one = a;
    one.sweep = 0;
    for (uint64_t base = 0; base < a.w_len; base += a.sweep) {   // (a sweep: one frame per thread, no stride)
        one.w0 = a.w0 + base;
        one.w_len = std::min<uint64_t>(a.sweep, a.w_len - base);
        const hipError_t e = launch_stage(one, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// Host loops of the track-history launches for the simulator, the same pattern as launch_input_range above.
__attribute__((weak)) hipError_t launch_track_tail(const TrackTailArgs &a, hipStream_t) {
    const uint64_t cap = a.mask + 1;
    for (uint64_t r = 0; r < a.rows; ++r)
        for (uint64_t i = 0; i < a.count; ++i)
            a.tail[r * cap + ((a.first + i) & a.mask)] = r < a.src_rows ? a.src[r * a.src_stride + a.col0 + i] : 0.0f;
    return hipSuccess;
}
__attribute__((weak)) hipError_t launch_ring_move(const RingMoveArgs &a, hipStream_t) {
    if (!ring_move_in_bounds(a)) return hipErrorInvalidValue;
    for (uint32_t i = 0; i < a.n_desc; ++i) {
        const RingMoveDesc &d = a.desc[i];
        for (uint64_t t = d.first; t != d.first + d.count; ++t)
            a.dst[(uint64_t)d.dst_row * (a.dst_mask + 1) + (t & a.dst_mask)] = a.src[(uint64_t)d.src_row * (a.src_mask + 1) + (t & a.src_mask)];
    }
    return hipSuccess;
}
// (no resident launches on the simulator: the serving rule and the tables are what it tests, through fr_plan_json)
__attribute__((weak)) hipError_t launch_bank_stream(StreamKernel, const StreamLaunchArgs &, hipStream_t) { return hipErrorNotSupported; }
__attribute__((weak)) hipError_t launch_track_window(const TrackWindowArgs &a, hipStream_t) {
    for (uint32_t r = 0; r < a.n_rows; ++r)
        for (uint64_t i = 0; i < a.back + a.n; ++i)
            a.dst[r][i] = i < a.back ? (a.tail[r] ? a.tail[r][(a.idx - a.back + i) & a.mask] : 0.0f) : (a.call[r] ? a.call[r][i - a.back] : 0.0f);
    return hipSuccess;
}

}  // namespace fr

using namespace fr;

struct fr_renderer {
    int device = 0;
    int mode = FR_MODE_AUTO;
    int semantics = FR_SEMANTICS_REFERENCE;
    uint64_t history_frames = 0;         // fr_config: 0 = keep everything since the last seek (the reference)
    hipStream_t stream = nullptr;
    Mirror mirror;
    // input history bookkeeping, same rules as reference.rs:47-75 (see oracle/ref_renderer.cpp)
    std::vector<InSlot> slots;
    uint64_t n_vecs = 0;
    struct Seg { uint64_t first, last, len; };
    std::vector<Seg> segs;
    uint64_t head = 0;
    Plan plan;
    DevBuf d_out, d_in_table, d_stack_node, d_stack_time, d_stack_val, d_bank_ws, d_tickets;
    // host-buffer entry point: input rows go up through pinned staging (one region per row, no sync between rows); the
    // finished frames come down through h_out_stage, which the kernels write DIRECTLY (mapped pinned memory: the stores
    // travel over PCIe while the launch is still computing), then one wait and one CPU copy into the caller's buffer
    PinnedBuf h_in_stage, h_out_stage;
    // Tracks (fr_set_track_inputs): input slots >= track_from are control-rate rows -- per-partial frequency / amplitude
    // envelopes -- that are NOT stored: the leaves of shape-matched voices read them from the call's own dense input matrix
    // (reference.rs:66-74: `inputs` is an Array2, one row per slot), 8 bytes per partial-frame straight from HBM.
    uint32_t track_from = 0xFFFFFFFFu;
    uint32_t dense_total_rows = 0;          // set around a dense call: rows of the caller's matrix
    const float *call_tracks = nullptr;     // row of slot 0 if the matrix started there (never dereferenced below track_from)
    uint64_t call_track_stride = 0, call_track_rows = 0;
    DevBuf d_tracks_stage;                  // host-buffer calls: the rows' copy in HBM
    // Track history (FR_TRACK_HISTORY = H frames, 0 = off): the last frames of every track row stay on the device, in a ring of
    // tail_cap (a power of two >= H) floats per row addressed by absolute frame (kernels.hpp TrackTailArgs), appended by every
    // call after all of its readers.  Readers through an input table (programs, the pull interpreter, template voices) get
    // this call's DevInput of the slot in track_dev; voices that read tracks over a look-back window read the ring itself.
    uint64_t track_history = 0, tail_cap = 0;
    DevBuf d_tail, d_track_win;
    uint32_t tail_rows = 0;
    uint64_t tail_end = 0;                  // frame after the last one the ring holds (a call that starts elsewhere seeks)
    uint64_t tail_launches = 0;             // track_tail_kernel launches of the last call (fr_plan_json)
    std::vector<std::pair<uint32_t, DevInput>> track_dev;   // (slot, this call's rows of it), by slot
    bool tail_on() const { return track_history != 0 && track_from != 0xFFFFFFFFu; }
    // shape-matched voices rendered in pieces (few voices x short call): the pieces' sums and the identity row list
    DevBuf d_chunk_ws, d_chunk_rows;
    uint32_t d_chunk_rows_n = 0;
    uint32_t stage_block_env = 0;           // FR_STAGE_BLOCK: iterations per block of compiled strided programs (A/B; 0 = the rule in build_plan)
    // FR_HOST_MAPPED (A/B): bit 0 = kernels write the output through the mapping, bit 1 = the bank kernel reads the
    // input row through the mapping; 0 = the staged copies of round 1 (H2D row, D2H of the whole buffer)
    bool host_out_mapped = false, host_rows_mapped = true;
    size_t host_small_bytes = 96u << 10; // FR_HOST_SMALL_KB: results up to this size leave through mapped pinned memory
    bool host_direct = true;             // FR_HOST_DIRECT=0: registered destinations are filled by a D2H copy like any other
    // Streamed output of the host entry point (plans whose rows all come straight from the time-major bank kernel): the
    // kernels store into mapped pinned memory and publish a flag per finished row; the host copies rows into the
    // caller's pageable buffer WHILE the launch is still computing the others.  FR_HOST_STREAM=0 turns it off.
    bool host_stream = true;
    PinnedBuf h_row_flags;               // [n_slots] u32: the call's sequence number once the row is complete
    DevBuf d_row_done;                   // per-voice tile counters of the launch (zero between launches)
    uint32_t host_seq = 0;
    std::vector<uint32_t> stream_pending;
    struct FlagOut { uint32_t *host_flags = nullptr; uint32_t *row_done = nullptr; uint32_t value = 0; } flag_out;
    // every output row is a voice of a bank launch that can publish its completion (bankplan.hpp BankPlan::publishes_rows)?
    bool can_stream_rows(uint32_t n_slots, uint64_t n_times) const {
        if (!host_stream || sharded() || !plan_current(n_slots) || plan.banks.empty()) return false;
        if (!plan.sp.progs.empty() || plan.sp.uses_rings() || !plan.pull_rows.empty() || !plan.sp.split.empty()) return false;
        size_t voices = 0;
        for (const BankStage &bs : plan.banks) {
            if (!plan_bank_launch(bs, n_times, true).publishes_rows) return false;
            voices += bs.grp.rows.size();
        }
        return voices == n_slots;   // (each row is written by exactly one voice: a row fed by nothing would be a program)
    }
    std::vector<std::pair<char *, size_t>> registered;   // fr_host_register: page-locked, device-visible host ranges
    bool host_trace = false;             // FR_HOST_TRACE=1: phase times of fr_fill_buffer on stderr at destroy
    double trace_us[3] = {0, 0, 0};
    uint64_t trace_n = 0;
    // Device-entry calls return before their work is done; a following call on ANOTHER stream (or the host entry
    // point, which uses the renderer's own stream) must still see this one's history, rings and plan uploads.
    hipEvent_t ev_last = nullptr;
    hipStream_t last_stream = nullptr;   // stream of the last asynchronous call while its work may still be running
    bool last_pending = false;
    bool last_independent = false;       // the last asynchronous call left nothing behind that a later call reads or reuses
    bool used_scratch = false;           // this call used a buffer shared between calls (the chunk workspace)
    bool host_pipelines = false;         // this call came on another stream than the previous, still pending one, and is independent of it
    bool overlapped_streams = false;     // independent calls were let loose on more than one stream since the last ordering point
    // Calls of a plan without delay lines, programs or pull rows touch only their own input rows and output buffer (and
    // append their own, disjoint part of the input history): on different streams they may overlap on the device.
    bool plan_is_stateless(uint32_t n_slots) const {
        return plan_current(n_slots) && !plan.sp.uses_rings() && plan.sp.progs.empty() && plan.pull_rows.empty() && plan.sp.split.empty() &&
               !tail_on();   // (every call appends to the track history)
    }
    void order_after_previous(hipStream_t st, bool this_independent = false) {
        if (!last_pending) return;
        if (overlapped_streams && !this_independent) {    // several streams may hold unfinished calls: wait for all of them
            HIP_CHECK(hipDeviceSynchronize());
            overlapped_streams = false;
            last_pending = false;
            return;
        }
        if (last_stream == st) return;                    // the usual case, one stream: nothing to do, nothing queued
        if (last_independent && this_independent) {       // independent work on another stream: let it overlap
            overlapped_streams = true;
            return;
        }
        // (an event recorded after EVERY call would put a barrier packet between consecutive kernels: ~2 us per call)
        if (!ev_last) HIP_CHECK(hipEventCreateWithFlags(&ev_last, hipEventDisableTiming));
        if (hipEventRecord(ev_last, last_stream) == hipSuccess) {
            HIP_CHECK(hipStreamWaitEvent(st, ev_last, 0));
        } else {                                          // the caller destroyed that stream: wait for whatever is left
            (void)hipGetLastError();
            HIP_CHECK(hipDeviceSynchronize());
        }
        last_pending = false;
    }
    void remember_async(hipStream_t st, bool independent) {
        last_independent = independent;
        last_stream = st;
        last_pending = true;
    }
    // ---- sharding (friendship_render.h fr_shard): this renderer is rank `shard.rank` of `shard.world`, one per GPU ----
    ShardSpec shard;
    uint32_t shard_flags = 0;
    uint64_t shard_epoch = 0;
    std::unique_ptr<Transport> rccl;     // the engine's own communicator (device to device over xGMI), or
    fr_comm host_comm{};                 // the host's callback (ranges staged through pinned memory)
    bool has_host_comm = false;
    DevBuf d_ws, d_xrecv;                // exchange workspace [tile][split voices][tile frames], receive buffer of the same shape
    // Time-tiled exchange: the window is cut into tiles; tile i's exchange runs on `xstream` while the bank kernels
    // of tile i + 1 run on the call's stream.  FR_EXCHANGE_TILES (most tiles per call, default 4; 1 = serial, as does the
    // FR_SHARD_SERIAL_EXCHANGE flag), FR_EXCHANGE_MIN_TILE (fewest frames worth a tile, default 1024).
    hipStream_t xstream = nullptr;
    std::vector<hipEvent_t> x_events;    // [tile] banks of the tile done (call's stream) ... and x_events.back(): exchange done (xstream)
    uint32_t x_max_tiles = 4, x_min_tile = 1024;
    bool x_tiles_explicit = false;       // either knob was set (environment or option): tile whatever the transport
    uint64_t exchange_bytes = 0;         // sent by this rank since the renderer was made (fr_plan_json)
    uint64_t exchange_calls = 0, exchange_tiles = 0;
    PinnedBuf h_xsend, h_xrecv;
    bool sharded() const { return shard.world > 1 && shard.mode != FR_SHARD_NONE; }
    void my_rows(uint32_t n_slots, uint32_t &lo, uint32_t &hi) const {
        lo = 0;
        hi = n_slots;
        if (sharded()) shard_row_range(shard.rank, shard.world, n_slots, lo, hi);
    }
    bool plan_current(uint32_t n_slots) const {
        return plan.valid && plan.version == mirror.version && plan.n_slots == n_slots && plan.shard_epoch == shard_epoch &&
               !(plan.jit_pending && plan.jit_epoch != jit_cache.epoch()) && !plan.observed_stale;
    }

    // Pairwise exchange with `peer` on stream st (device pointers, counts in floats).
    void xfer(uint32_t peer, const float *d_send, size_t n_send, float *d_recv, size_t n_recv, hipStream_t st) {
        if (!n_send && !n_recv) return;
        if (rccl) { rccl->sendrecv(peer, d_send, n_send, d_recv, n_recv, st); return; }
        if (!has_host_comm) throw Error(FR_ERR_COMM, "the sharded plan needs an exchange but fr_set_shard was given no transport");
        h_xsend.ensure(n_send * sizeof(float));
        h_xrecv.ensure(n_recv * sizeof(float));
        if (n_send) HIP_CHECK(hipMemcpyAsync(h_xsend.p, d_send, n_send * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));   // the send range is on the host; an earlier upload from h_xrecv is done
        const int32_t rc = host_comm.sendrecv(host_comm.ctx, peer, h_xsend.p, n_send * sizeof(float), h_xrecv.p, n_recv * sizeof(float));
        if (rc != 0) throw Error(FR_ERR_COMM, "transport callback failed with code " + std::to_string(rc) + " exchanging with rank " + std::to_string(peer));
        if (n_recv) HIP_CHECK(hipMemcpyAsync(d_recv, h_xrecv.p, n_recv * sizeof(float), hipMemcpyHostToDevice, st));
    }

    // The one exchange step of the path (FR_SHARD_PARTIALS): recursive halving over the ranks.  The workspace holds, for
    // every split voice, this rank's sub-tree sum over the window; rows are ordered by the owner's bits, lowest bit
    // first.  Step j pairs rank with rank ^ 2^j: each keeps the rows whose owner agrees with it in bit j, sends the
    // rest, and adds what it receives -- left operand from the rank whose bit j is 0: that is the voice's Sum2 node j
    // levels above the sub-tree roots, evaluated with the graph's own operands in the graph's own order.  After
    // log2(world) steps each rank holds the finished voices it owns; the last add stores them where the unsharded
    // plan would (ring or output row).
    // One time tile of the window: frames [x0 + off, x0 + off + len) of every split voice.  The workspaces are tile-major
    // ([tile][split voice][tile frame]), so a tile's rows are contiguous ranges for the transport and tiles in flight on the
    // exchange stream never share a byte with the tile the bank kernels are writing.
    void run_exchange(float *d_dst, uint64_t n_times, uint64_t idx, uint64_t x0, uint64_t off, uint64_t len, hipStream_t st) {
        const std::vector<SplitVoice> &sv = plan.sp.split;
        uint32_t k = 0;
        while ((1u << k) < shard.world) ++k;
        size_t lo = 0, hi = sv.size();
        float *ws = d_ws.as<float>() + sv.size() * off;
        float *rbuf = d_xrecv.as<float>() + sv.size() * off;
        for (uint32_t j = 0; j < k; ++j) {
            const uint32_t bit = 1u << j, peer = shard.rank ^ bit;
            size_t mid = lo;
            while (mid < hi && !(sv[mid].owner & bit)) ++mid;
            const bool upper = (shard.rank & bit) != 0;
            const size_t keep_lo = upper ? mid : lo, keep_hi = upper ? hi : mid;
            const size_t send_lo = upper ? lo : mid, send_hi = upper ? mid : hi;
            xfer(peer, ws + send_lo * len, (send_hi - send_lo) * len, rbuf, (keep_hi - keep_lo) * len, st);
            exchange_bytes += (send_hi - send_lo) * len * sizeof(float);
            ShardCombineArgs c{};
            float *mine = ws + keep_lo * len;
            c.lo = upper ? rbuf : mine;
            c.hi = upper ? mine : rbuf;
            c.n_rows = (uint32_t)(keep_hi - keep_lo);
            c.len = len;
            if (j + 1 < k) {
                c.dst_ws = mine;
            } else {
                // the finished voices go where the unsharded plan puts them: ring frame x0 + off + t, or -- frames of the call
                // only, the look-back part of a window is not output -- column x0 + off + t - idx of the output row
                const uint64_t skip = idx - x0;                      // window frames before the call's first frame
                c.dst = plan.d_split_dst.as<uint32_t>() + keep_lo;
                c.out = d_dst + (off > skip ? off - skip : 0);
                c.out_stride = n_times;
                c.out_skip = skip > off ? skip - off : 0;
                c.rings = d_rings.as<float>();
                c.ring_mask = ring_cap ? ring_cap - 1 : 0;
                c.ring_t0 = x0 + off;
            }
            Scope sc(this, &t_stage, st);
            HIP_CHECK(launch_shard_combine(c, st));
            sc.done();
            lo = keep_lo;
            hi = keep_hi;
        }
        for (size_t i = lo; i < hi; ++i)
            if (sv[i].owner != shard.rank) throw Error(FR_ERR_COMM, "internal: exchange order does not match voice ownership");
    }

    // FR_SHARD_GATHER: every rank's rows to rank 0's buffer.
    void gather_rows(float *d_dst, uint32_t n_slots, uint64_t n_times, hipStream_t st) {
        if (!sharded() || !(shard_flags & FR_SHARD_GATHER)) return;
        if (shard.rank == 0) {
            for (uint32_t p = 1; p < shard.world; ++p) {
                uint32_t lo, hi;
                shard_row_range(p, shard.world, n_slots, lo, hi);
                xfer(p, nullptr, 0, d_dst + (size_t)lo * n_times, (size_t)(hi - lo) * n_times, st);
            }
        } else {
            uint32_t lo, hi;
            my_rows(n_slots, lo, hi);
            xfer(0, d_dst + (size_t)lo * n_times, (size_t)(hi - lo) * n_times, nullptr, 0, st);
        }
    }

    bool timing = false;
    // A/B switches (per-renderer options or the environment, read at create: the option table below; defaults are the
    // measured best):
    int64_t option_value[N_OPTIONS];
    uint8_t option_source[N_OPTIONS];
    std::string options_json_cache;
    BankTuning bank_tune;                // FR_BANK_*, FR_SHORT_*, FR_JIT_CHUNKS, FR_JIT_CHUNK_TARGET: this renderer's bank launch rule
    // A bank group's launch over `n_times` frames in this call (bankplan.hpp): the launch itself, the input store's row
    // deferral and the streamed host output all ask this, so they agree by construction.
    BankPlan plan_bank_launch(const BankStage &bs, uint64_t n_times, bool row_flags, uint32_t n_voices = UINT32_MAX) const {
        return plan_bank(bs.grp, BankCall{n_times, host_pipelines, row_flags, bs.jit && bs.jit->fn_multi}, bank_tune, n_voices);
    }
    bool jit_fma = true;                 // FR_JIT_FMA=0: generated leaves without the fused multiply-add fold (jit.hpp)
    unsigned lower_threads = 1;          // FR_LOWER_THREADS, FR_LOWER_PAR_MIN_NODES, FR_LOWER_PAR_MIN_EDIT (Lowering::set_parallel)
    size_t lower_min_nodes = 0, lower_min_edit = 0;
    std::vector<BankLaunchNote> bank_launches;   // the last call's (fr_plan_json), at most 256
    std::vector<StageLaunchNote> stage_launches; // (likewise)
    const char *bank_form = "call";      // what the bank launches being issued are for (BankLaunchNote::form)
    void note_bank_launch(const BankPlan &bp, const BankStage &bs, uint32_t voices, uint64_t frames, bool row_flags) {
        const uint32_t partials = bs.grp.general ? bs.grp.max_leaves : 1u << bs.grp.log2_p;
        if (bank_launches.size() < 256)
            bank_launches.push_back({bp, voices, partials, frames, bs.grp.log2_p, bank_tune.leaf_variant, row_flags, bank_form});
    }
    // Block streaming (fr_stream_*): one resident launch renders 64-frame blocks on a doorbell (kernels.hpp BankStreamCtl).
    // A plan with programs (FR_STREAM_PROGRAMS, streamplan.hpp) is launched with its first block and again with every block
    // that does not continue the previous one, after the rings were brought up to that block's first frame.
    struct Stream {
        struct Open {                    // the open stream: opening and closing one replaces the whole object
            bool prog = false;           // it is of the program path
            bool launched = false;       // its resident launch is running
            bool have_last = false;
            uint32_t seq = 0, slots = 0;
            uint64_t head = 0;           // first frame after the last streamed block
            StreamLaunch launch;         // how it is launched (streamplan.hpp): everyone reads this and decides nothing
            StreamPlan plan;
            StreamRows rows;             // the input store's rules for its rows, without the samples (streamrows.hpp)
            // FR_STREAM_GENERAL: per plan bank the word offsets in d_sched of the one-item schedule (groups, group_off) built for a
            // balanced 32- or 64-partial bank (SIZE_MAX: the bank has none of its own here)
            std::vector<std::pair<size_t, size_t>> sched_at;
            // FR_STREAM_STORE (streamstore.hpp): the launch appends the streamed rows to the input store and the renderer's books
            // follow block by block; `streamed`: the slots of the launch's rows, in order; `rows_open`: `rows` are the store's books
            bool store = false, rows_open = false, continued = false;
            uint32_t relaunches = 0;
            std::vector<StoreStreamed> streamed;
        } now;
        bool open = false;
        // what outlives a stream: the buffers (they only grow), the last resident launch's kernel (fr_plan_json "stream"), the trace
        PinnedBuf h_ctl, h_out;
        DevBuf d_dev, d_progs, d_vfirst, d_sched, d_instrs, d_hist;   // (d_instrs: StreamLaunch::own_instrs; d_hist: StreamLaunch::hist_cap)
        PinnedBuf h_trk;                 // FR_STREAM_TRACKS: the staging of a block's track rows, [StreamPlan::track_rows][64] floats (kernels.hpp StreamTrackArgs)
        DevBuf d_leaf;                   // FR_STREAM_LEAVES: the leaf banks' programs, bank after bank (StreamPlan::leaf_progs; LEAF_IN by streamed row)
        StreamKernel last_kernel = StreamKernel::none;
        double trace_us[2] = {0, 0};
        uint64_t trace_n = 0;
    } strm;
    uint32_t stream_idle_ms = BANK_STREAM_IDLE_MS;   // FR_STREAM_IDLE_MS (tests shorten it)
    int device_cus = 0;
    // The in-launch combine's arrival counters (d_tickets) and the row-completion counters (d_row_done) are "all zero
    // between launches": every launch that uses them leaves them so.  A launch that ended abnormally may not have: whatever
    // can leave them dirty sets this, and the next user clears them before its launch.
    bool counters_dirty = false;
    void clean_counters(hipStream_t st) {
        if (!counters_dirty) return;
        if (d_tickets.p) HIP_CHECK(hipMemsetAsync(d_tickets.p, 0, d_tickets.bytes, st));
        if (d_row_done.p) HIP_CHECK(hipMemsetAsync(d_row_done.p, 0, d_row_done.bytes, st));
        counters_dirty = false;
    }
    // `words` arrival counters for a launch with an in-launch combine: zero between launches (the kernel resets them).
    uint32_t *ticket_counters(size_t words, hipStream_t st) {
        const size_t need = words * sizeof(uint32_t);
        clean_counters(st);
        if (need > d_tickets.bytes) {
            d_tickets.ensure(need * 2);
            HIP_CHECK(hipMemsetAsync(d_tickets.p, 0, d_tickets.bytes, st));
        }
        return d_tickets.as<uint32_t>();
    }
    // FR_STREAM_PROGRAMS, _BUS, _INPUTS, _LOOPS, _BANKS, _GENERAL, _DYN, _HISTORY, _EFFECTS, _STORE, _TAPS, _SWEEP, _LEAVES, _TRACKS (the options table says what each serves; streamplan.hpp StreamEnv)
    bool stream_programs = false, stream_bus = false, stream_inputs = false, stream_loops = false, stream_banks = false, stream_general = false, stream_dyn = false,
         stream_history = false, stream_effects = false, stream_store = false, stream_taps = false, stream_sweep = false, stream_leaves = false, stream_tracks = false;
    // Why FR_STREAM_STORE does nothing for this renderer ("": it acts; streamstore.hpp).  Declared track slots make it inert unless
    // the stream itself reads tracks (FR_STREAM_TRACKS on its two options): then the rows below the first track slot are stored
    // like any streamed row and the tracks, as in fr_fill_buffer_dense, are not.
    bool stream_tracks_act() const { return stream_tracks && stream_leaves && stream_programs; }
    std::string stream_store_inert_now() const { return stream_store_inert(delay_observed, track_from != 0xFFFFFFFFu && !stream_tracks_act()); }
    std::vector<const BankLaunch *> stream_bank_list() const {
        std::vector<const BankLaunch *> banks;
        for (const BankStage &bs : plan.banks) banks.push_back(&bs.grp);
        return banks;
    }
    StreamEnv stream_env() const {
        StreamEnv env;
        env.n_slots = plan.n_slots;
        env.device_cus = (uint32_t)std::max(device_cus, 0);
        env.leaf_variant = bank_tune.leaf_variant;
        env.pull_mode = mode == FR_MODE_PULL;
        env.sharded = sharded();
        env.track_history = tail_on();
        env.programs = stream_programs; env.bus = stream_bus; env.inputs = stream_inputs;
        env.banks = stream_banks; env.loops = stream_loops; env.general = stream_general; env.dyn = stream_dyn;
        env.history = stream_history;
        env.effects = stream_effects;
        env.taps = stream_taps;
        env.sweep = stream_sweep;
        env.leaves = stream_leaves;
        env.tracks = stream_tracks;
        env.track_from = track_from;
        env.store = stream_store && stream_programs && stream_store_inert_now().empty();
        return env;
    }
    StreamPlan plan_stream_now() const { return plan_stream(plan.sp, stream_bank_list(), stream_env()); }
    // Rings the stop and waits for the resident launch to end.  `clean`: the launch was answering when the stop was rung
    // (every block it took was finished).  Otherwise some chunks of a voice may have taken their ticket and others never
    // run: the counters are cleared before anyone uses them again.  Returns whether the stop WAS clean: false also when the wait
    // for the launch's end failed.
    bool stop_resident(bool clean) {
        if (strm.now.launched) {
            const StreamDoorbell bell = stream_doorbell(strm.h_ctl.p, strm.now.launch.rows_doorbell);   // (the stop goes to every row)
            for (size_t i = 0; i < bell.n_words; ++i) __atomic_store_n(&bell.words[i], (unsigned long long)BANK_STREAM_STOP << 32, __ATOMIC_RELEASE);
            if (hipStreamSynchronize(stream) != hipSuccess) { (void)hipGetLastError(); clean = false; }   // the kernel sees the stop within a poll, or ends itself after its bound
        }
        strm.now.launched = false;
        strm.now.have_last = false;
        if (!clean) counters_dirty = true;
        return clean;
    }
    void end_stream(bool clean = true) {
        if (!strm.open) return;
        clean = stop_resident(clean);
        if (strm.now.store) {
            // the stream stored what it was fed and every answered block is in the renderer's books (commit_streamed_block): the
            // renderer stands as after an ordinary call that ended at `head`.  An unanswered block: its rows are not in the books,
            // the rings may hold part of it -- the next call rebuilds them from the history.
            if (!clean) { plan.stage_valid = false; ring_table.valid = false; }
            strm.open = false;
            strm.now = Stream::Open{};
            return;
        }
        if (strm.now.prog) {                     // the rings moved on with frames the input store never saw
            plan.stage_valid = false;
            ring_table.valid = false;
        }
        strm.open = false;
        strm.now = Stream::Open{};
        head = UINT64_MAX;                       // the streamed frames were not stored: whatever comes next is a seek
    }
    void ensure_stream_buffers(const StreamLaunch &l, uint32_t n_slots) {
        const StreamDoorbell bell = stream_doorbell(nullptr, l.rows_doorbell);
        strm.h_ctl.ensure(bell.ctl_bytes);
        strm.h_out.ensure((size_t)n_slots * 64 * sizeof(float));
        strm.d_dev.ensure(bell.dev_bytes);
    }
    void open_stream(Stream::Open &&o, uint32_t n_slots) {
        o.slots = n_slots;
        o.rows.open(n_vecs);
        strm.now = std::move(o);
        strm.open = true;
        last_pending = false;
    }
    // An answered block of a stream that stores its rows: the books an ordinary call ending at idx + n_times leaves -- the fed
    // slots' lengths, the segments and the vector count (streamstore.hpp), head, and the rings' end.
    void commit_streamed_block(uint32_t rows_fed, uint64_t idx, uint64_t n_times) {
        stream_store_commit(slots, segs, n_vecs, strm.now.rows, rows_fed, idx, n_times);
        head = idx + n_times;
        if (!plan.sp.uses_rings()) return;
        plan.stage_valid = true;
        plan.stage_end = head;
        if (ring_keep && ring_state.inert.empty() && ring_table.valid) {   // (as commit_rings: the oldest frames of a full ring are gone)
            ring_table.end = head;
            const uint64_t oldest = head > ring_cap ? head - ring_cap : 0;
            for (RingEntry &e : ring_table.rings) e.valid_from = std::max(e.valid_from, oldest);
        }
    }
    // The last stored value of every fed slot that holds samples (one small D2H each, before anything is resident): what an empty
    // row of the first continuing block pads with.
    std::vector<float> last_stored_values() {
        std::vector<float> last(slots.size(), 0.0f);
        bool any = false;
        for (size_t r = 0; r < slots.size(); ++r) {
            const InSlot &s = slots[r];
            if (!s.fed || s.len <= s.base || !s.buf.p) continue;
            HIP_CHECK(hipMemcpyAsync(&last[r], s.buf.as<float>() + (s.len - s.base - 1), sizeof(float), hipMemcpyDeviceToHost, stream));
            any = true;
        }
        if (any) HIP_CHECK(hipStreamSynchronize(stream));
        return last;
    }
    // The BankArgs of a resident launch over the one bank `bs`; null: the banks travel as a table, and what BankArgs says of one
    // bank (params, rows, log2_p, chunk_log2, fast_ok) is not read and stays zero.
    BankArgs stream_bank_args(const BankStage *bs, uint32_t voices, uint32_t chunk_log2, uint32_t chunks) {
        BankArgs a{};
        if (bs) {
            a.params = bs->d_params.as<float2>();
            a.rows = bs->d_rows.as<uint32_t>();
            a.log2_p = bs->grp.log2_p;
            a.fast_ok = bs->grp.fast_ok ? 1u : 0u;
            a.chunk_log2 = chunk_log2;
        }
        a.n_voices = voices; a.n_times = 64; a.leaf_variant = 1;
        a.small_call = 2; a.waves_per_group = 16; a.frames_per_lane = 1;   // (the short-call kernel's shape)
        if (chunks > 1) {
            d_bank_ws.ensure((size_t)voices * chunks * 64 * sizeof(float));
            a.ws = d_bank_ws.as<float>();
            a.tickets = ticket_counters((size_t)voices * BANK_TICKET_STRIDE, stream);
        }
        a.out = strm.h_out.as_dev<float>(); a.out_stride = 64;
        return a;
    }
    // The resident launch of stream `o` from a clean control block (the previous launch's doorbell and stop are still in the words);
    // `x`: the kernel's arguments, without what is filled in here.
    void launch_resident(Stream::Open &o, StreamLaunchArgs &x) {
        const StreamLaunch &l = o.launch;
        const StreamDoorbell bell = stream_doorbell(strm.h_ctl.p, l.rows_doorbell);
        std::memset(strm.h_ctl.p, 0, bell.ctl_bytes);
        HIP_CHECK(hipMemsetAsync(strm.d_dev.p, 0, bell.dev_bytes, stream));
        x.n_rows = l.n_rows;
        x.max_stride = l.max_stride; x.max_loads = l.max_loads; x.max_stores = l.max_stores;
        x.ctl_dev = strm.h_ctl.dev; x.dev = strm.d_dev.p; x.idle_ms = stream_idle_ms;
        HIP_CHECK(launch_bank_stream(l.kernel, x, stream));
        strm.last_kernel = l.kernel;
        o.launched = true;
        last_pending = false;
    }
    void begin_program_stream(uint32_t n_slots);
    void upload_stream_programs(const StreamPlan &s, const StreamLaunch &l, const std::vector<uint32_t> &row_slots, uint32_t n_slots);
    void begin_program_stream_rest(Stream::Open &&o, StreamPlan &&s, uint32_t n_slots);
    void seek_program_stream(uint64_t idx);
    void start_resident(uint64_t idx, bool empty_history);
    void launch_store_stream(uint64_t idx, uint32_t rows_fed, bool seek);
    void fill_stream_history(uint64_t idx);
    bool allow_jit = true;               // FR_JIT=0: no hipRTC specialisation (those voices run as programs / pull)
    bool allow_template = true;          // FR_BANK_TEMPLATE=0: template voices go through the JIT path literally
    bool fused_strided_ok = true;        // FR_STAGE_STRIDED=0: a long steady call of the fused form as one launch per sub-window (A/B)
    int stage_jit_mode = 1;              // FR_STAGE_JIT=0: programs always interpreted; 1: compiled when >= 4 programs share
                                         // a skeleton on average; 2 ("force"): compiled whenever they fit one kernel
    JitCache jit_cache;
    bool jit_async_configured = true;    // fr_config: hipRTC on the worker thread unless FR_CONFIG_SYNC_COMPILE
    Lowering lowering;                   // lowered graph, kept up to date across edits
    std::unique_ptr<BankMatcher> matcher;   // voice recognition memo over lowering's graph (same generation)
    uint64_t matcher_gen = 0;
    uint64_t plans_built = 0, plans_incremental = 0;
    TimerClass t_bank, t_pull, t_stage;
    DevBuf d_rings, d_in_table_stage;
    uint64_t ring_cap = 0;               // floats per ring (power of two)
    // ---- kept delay lines (FR_RING_KEEP) ----------------------------------------------------------------------------
    // What d_rings holds, per physical ring, outliving the plan: the lowering generation and the key of the function the ring
    // holds (StagedPlan::ring_node, then ring_fb: equal keys in one generation are the same function of the same history) and
    // the oldest frame it holds for that key; `end` is the frame after the last one every ring holds.  The first call after a
    // re-plan keeps the rings of the new plan it finds here with enough frames for their look-back, moves them to their new
    // rows (ring_move_kernel) and brings only the others up to idx before it runs as a steady call.
    bool ring_keep = false;
    // Loop tiles (FR_LOOP_TILES, callplan.hpp loop_tile): the strided launches of feedback plans of short strides render tiles
    // staged in LDS.  `loop_tiles_given`: the option was set (either way): fr_plan_json then shows "loop_tiles".
    bool loop_tiles = false, loop_tiles_given = false;
    // Feedback through a Delay of a signal amount (FR_LOOP_DYN; callplan.hpp loop_sweep): 0 = such loops are FR_ERR_CYCLE, 1 = their
    // plans run on stage_sweep_kernel, 2 = on stage_kernel a window of W frames at a time.  `loop_dyn_given`: the option was set
    // (to anything): fr_plan_json then shows "loop_dyn".
    int loop_dyn = 0;
    bool loop_dyn_given = false;
    struct RingEntry { uint64_t generation; std::vector<uint32_t> key; uint64_t valid_from; };
    struct RingTable {
        bool valid = false;
        uint64_t end = 0, shard_epoch = 0;
        std::vector<RingEntry> rings;
    } ring_table;
    struct RingState { uint32_t kept = 0, rebuilt = 0, moved = 0, move_launches = 0; uint64_t repair_from = 0; std::string inert; } ring_state;
    bool rings_touched = false;          // the call in hand has reached execute(): its launches may have written rings
    PinnedBuf h_ring_desc;               // the move's descriptors (the kernel reads them through the mapping)
    hipEvent_t ev_ring_move = nullptr;   // ... free for the next move once this has passed
    // What the repair launches (repair_rings): bank voices as runs [first, first + count) of a stage's voices, programs as runs
    // of plan.sp.progs level by level, all over [from, idx); `replay`: a feedback plan's loops, from frame 0 in chunks.
    struct RingRepair {
        bool replay = false;
        uint64_t from = 0;
        struct Run { uint32_t stage, first, count; };
        std::vector<Run> voices;
        std::vector<std::vector<std::pair<uint32_t, uint32_t>>> levels;   // per level: (first program, count)
        bool empty() const { return voices.empty() && levels.empty(); }
    };
    // Why the option does nothing for this plan ("" = it acts): everything is rebuilt as without it.
    std::string ring_keep_inert() const {
        const StagedPlan &sp = plan.sp;
        if (sharded() && shard.mode == FR_SHARD_PARTIALS) return "partial-block sharding";
        if (!sp.split.empty()) return "partial-block sharding";
        if (!sp.track_window_slots.empty()) return "track history";
        for (const BankStage &bs : plan.banks)
            if (bs.grp.tracks && bs.grp.to_ring) return "track history";
        // (A repair, like the window rebuild without the option, reads the stored inputs over the look-back; with a bounded
        //  history those reads return 0.0 below history_floor, which only ever rises.  A ring kept from before the floor rose
        //  holds what the full history gave, a rebuilt one what the floored history gives: the option would change bits.)
        if (history_frames != 0) return "bounded input history";
        if (!sp.uses_rings()) return "no delay lines";
        // (what a kept loop's repair replays is decided per ring by the constant delays its readers use; a sweep plan's are signals)
        if (sp.fused_sweep) return "a loop delays by a signal amount";
        return "";
    }
    static std::vector<uint32_t> ring_key(const StagedPlan &sp, uint32_t r) {
        std::vector<uint32_t> key{sp.ring_node[r]};
        if (r < sp.ring_fb.size()) key.insert(key.end(), sp.ring_fb[r].begin(), sp.ring_fb[r].end());
        return key;
    }
    // build_plan: the planner numbers rings by node id, and an edit appends nodes, so the rings behind an edited node would all
    // shift by a few rows.  Rings the table already holds get the row they are in and the new ones the rows left over (a
    // permutation of the plan's numbering, applied before anything is uploaded or compiled): a knob turn then moves nothing.
    void renumber_rings(StagedPlan &sp) const {
        const uint32_t n = sp.n_rings;
        if (!ring_keep || n == 0 || !sp.split.empty() || ring_table.rings.empty()) return;
        const uint64_t gen = lowering.generation();
        std::map<std::vector<uint32_t>, uint32_t> held;
        for (uint32_t o = 0; o < ring_table.rings.size() && o < n; ++o)
            if (ring_table.rings[o].generation == gen) held.emplace(ring_table.rings[o].key, o);
        std::vector<uint32_t> perm(n, UINT32_MAX);
        std::vector<uint8_t> used(n, 0);
        for (uint32_t r = 0; r < n; ++r) {
            auto it = held.find(ring_key(sp, r));
            if (it != held.end() && !used[it->second]) { perm[r] = it->second; used[it->second] = 1; }
        }
        uint32_t free_row = 0;
        for (uint32_t r = 0; r < n; ++r) {
            if (perm[r] != UINT32_MAX) continue;
            while (used[free_row]) ++free_row;
            perm[r] = free_row;
            used[free_row] = 1;
        }
        for (StageInstr &in : sp.instrs)
            if (in.op == S_READ || in.op == S_READ_DYN || in.op == S_STORE) in.buf = perm[in.buf];
        for (StageProg &pg : sp.progs)
            if (pg.dst_ring < n) pg.dst_ring = perm[pg.dst_ring];
        for (BankLaunch &bl : sp.banks)
            if (bl.to_ring) for (uint32_t &row : bl.rows) row = perm[row];
        for (std::vector<uint32_t> &pr : sp.prog_rings) {
            for (uint32_t &r : pr) r = perm[r];
            std::sort(pr.begin(), pr.end());
        }
        std::vector<uint32_t> node(n);
        std::vector<uint64_t> lb(n);
        std::vector<std::vector<uint32_t>> fb(sp.ring_fb.size());
        for (uint32_t r = 0; r < n; ++r) {
            node[perm[r]] = sp.ring_node[r];
            lb[perm[r]] = sp.ring_lookback[r];
            if (r < sp.ring_fb.size()) fb[perm[r]] = std::move(sp.ring_fb[r]);
        }
        sp.ring_node = std::move(node);
        sp.ring_lookback = std::move(lb);
        sp.ring_fb = std::move(fb);
    }
    static bool ring_in(const std::vector<uint8_t> &set, const std::vector<uint32_t> &rings) {
        for (uint32_t r : rings) if (set[r]) return true;
        return false;
    }
    static void add_run(std::vector<std::pair<uint32_t, uint32_t>> &runs, uint32_t i) {
        if (!runs.empty() && runs.back().first + runs.back().second == i) ++runs.back().second;
        else runs.push_back({i, 1});
    }
    // The first call of a plan whose rings are not known to be current (a new plan, a longer call than any before, a seek, a
    // failed call): which rings of the table serve the new plan, the move, and what must be launched to rebuild the rest.
    // Leaves d_rings / ring_cap as the call needs them and the table describing the new plan's rings as they will be at idx.
    RingRepair keep_rings(uint64_t cap_needed, uint64_t idx, bool table_was_valid, hipStream_t st) {
        const StagedPlan &sp = plan.sp;
        const uint32_t n = sp.n_rings;
        const uint64_t gen = lowering.generation();
        const bool live = table_was_valid && ring_table.end == idx && ring_table.shard_epoch == shard_epoch && d_rings.p && ring_cap;
        std::vector<std::vector<uint32_t>> keys(n);
        for (uint32_t r = 0; r < n; ++r) keys[r] = ring_key(sp, r);
        std::vector<int64_t> src(n, -1);
        if (live) {
            std::map<std::vector<uint32_t>, uint32_t> held;
            for (uint32_t o = 0; o < ring_table.rings.size(); ++o)
                if (ring_table.rings[o].generation == gen) held.emplace(ring_table.rings[o].key, o);
            for (uint32_t r = 0; r < n; ++r) {
                auto it = held.find(keys[r]);
                const uint64_t lb = sp.ring_lookback[r];
                if (it != held.end() && ring_table.rings[it->second].valid_from <= (idx > lb ? idx - lb : 0)) src[r] = it->second;
            }
        }
        uint32_t kept = 0;
        bool permuted = false;
        for (uint32_t r = 0; r < n; ++r)
            if (src[r] >= 0) { ++kept; permuted = permuted || src[r] != (int64_t)r; }
        const uint64_t new_cap = std::max(ring_cap, cap_needed);
        const size_t new_bytes = (size_t)n * new_cap * sizeof(float);
        std::vector<RingEntry> now(n);
        for (uint32_t r = 0; r < n; ++r) now[r] = RingEntry{gen, std::move(keys[r]), src[r] >= 0 ? ring_table.rings[(size_t)src[r]].valid_from : UINT64_MAX};
        ring_state.kept = kept;
        ring_state.rebuilt = n - kept;
        if (kept && (permuted || new_cap != ring_cap || new_bytes > d_rings.bytes)) {
            // rows permute and capacities differ: into a second allocation, the old one retired behind the stream
            DevBuf nb;
            nb.ensure(new_bytes + new_bytes / 4 + 8 * new_cap * sizeof(float));   // (rows to spare: the next note-on moves nothing)
            // (the one host wait of the path, on an event and not on the device: the previous move -- at least one call ago,
            //  moves are rare -- must have read its descriptors before the pinned buffer is written again; normally long past)
            if (ev_ring_move) HIP_CHECK(hipEventSynchronize(ev_ring_move));
            else HIP_CHECK(hipEventCreateWithFlags(&ev_ring_move, hipEventDisableTiming));
            h_ring_desc.ensure((size_t)kept * sizeof(RingMoveDesc));
            RingMoveDesc *desc = h_ring_desc.as<RingMoveDesc>();
            const uint64_t reach = std::min(ring_cap, new_cap);
            uint32_t nd = 0;
            for (uint32_t r = 0; r < n; ++r) {
                if (src[r] < 0) continue;
                const uint64_t first = std::max(now[r].valid_from, idx > reach ? idx - reach : 0);
                now[r].valid_from = first;
                if (first < idx) desc[nd++] = RingMoveDesc{(uint32_t)src[r], r, first, idx - first};
            }
            RingMoveArgs a{};
            a.src = d_rings.as<float>();
            a.dst = nb.as<float>();
            a.src_mask = ring_cap - 1;
            a.dst_mask = new_cap - 1;
            a.src_rows = (uint32_t)std::min<uint64_t>(ring_table.rings.size(), d_rings.bytes / (ring_cap * sizeof(float)));
            a.dst_rows = n;
            a.desc = h_ring_desc.as_dev<RingMoveDesc>();
            a.host_desc = desc;
            a.n_desc = nd;
            if (nd) {
                Scope sc(this, &t_stage, st);
                HIP_CHECK(launch_ring_move(a, st));
                sc.done();
                HIP_CHECK(hipEventRecord(ev_ring_move, st));
                ring_state.move_launches = 1;
            }
            ring_state.moved = nd;
            bury(std::move(d_rings), st);
            d_rings = std::move(nb);
        } else if (new_bytes > d_rings.bytes) {
            d_rings.ensure(new_bytes + new_bytes / 4 + 8 * new_cap * sizeof(float));   // (nothing kept: nothing to carry over)
        }
        ring_cap = new_cap;

        // what to rebuild
        RingRepair rp;
        rp.from = idx;
        std::vector<uint8_t> need(n, 0);
        uint64_t deepest = 0;
        bool any = false;
        for (uint32_t r = 0; r < n; ++r) {
            if (src[r] >= 0) continue;
            now[r].valid_from = idx;                 // (until something below writes older frames of it)
            if (sp.ring_lookback[r] == 0) continue;  // read at its own frame only: the call itself fills it
            need[r] = 1;
            any = true;
            deepest = std::max(deepest, sp.ring_lookback[r]);
        }
        if (idx == 0) {                              // nothing before frame 0: every ring is current, and stays valid from 0
            for (RingEntry &e : now) e.valid_from = 0;
            any = false;
        }
        std::vector<uint8_t> bank_ring(n, 0);
        for (const BankStage &bs : plan.banks)
            if (bs.grp.to_ring) for (uint32_t row : bs.grp.rows) bank_ring[row] = 1;
        auto add_voices = [&](const std::vector<uint8_t> &want) {
            for (uint32_t b = 0; b < plan.banks.size(); ++b) {
                const BankLaunch &g = plan.banks[b].grp;
                if (!g.to_ring) continue;
                std::vector<std::pair<uint32_t, uint32_t>> runs;
                for (uint32_t v = 0; v < g.rows.size(); ++v) if (want[g.rows[v]]) add_run(runs, v);
                // (the schedule kernel's voices index shared tables: all of them, rewriting the kept ones with what they hold)
                if (g.general && !runs.empty()) runs.assign(1, {0u, (uint32_t)g.rows.size()});
                for (auto &run : runs) rp.voices.push_back({b, run.first, run.second});
            }
        };
        if (any && !sp.feedback) {
            rp.from = idx - std::min(idx, deepest);
            add_voices(need);
            // the oldest frame each written ring is right from: a bank's from the window's start (it reads inputs only), a
            // program's as far as everything it reads reaches (frames before 0 are zeros by definition)
            for (uint32_t r = 0; r < n; ++r) if (need[r] && bank_ring[r]) now[r].valid_from = rp.from;
            const size_t n_levels = sp.level_first.empty() ? 0 : sp.level_first.size() - 1;
            for (size_t l = 0; l < n_levels; ++l) {
                std::vector<std::pair<uint32_t, uint32_t>> runs;
                for (uint32_t i = sp.level_first[l]; i < sp.level_first[l + 1]; ++i) {
                    if (!ring_in(need, sp.prog_rings[i])) continue;
                    add_run(runs, i);
                    const StageProg &pg = sp.progs[i];
                    uint64_t from = rp.from;
                    for (uint32_t k = 0; k < pg.n_instr; ++k) {
                        const StageInstr &in = sp.instrs[pg.first_instr + k];
                        if (in.op != S_READ && in.op != S_READ_DYN) continue;
                        const uint64_t vf = now[in.buf].valid_from;
                        if (vf != 0) from = std::max(from, vf + in.d_lo);
                    }
                    for (uint32_t r : sp.prog_rings[i]) now[r].valid_from = std::min(from, idx);
                }
                if (!runs.empty()) rp.levels.push_back(std::move(runs));
            }
        } else if (any) {
            // Feedback: a loop's state at idx is a function of every frame since 0.  The programs that store a ring to rebuild
            // are replayed from 0, together with everything upstream they read while replaying (kept rings hold their last
            // frames only; the replay rewrites them and they end where they were).
            rp.replay = true;
            rp.from = 0;
            const uint32_t f0 = sp.fused_first, f1 = sp.fused_first + sp.fused_count;
            std::vector<int64_t> stored_by(n, -1);
            for (uint32_t i = f0; i < f1; ++i) for (uint32_t r : sp.prog_rings[i]) stored_by[r] = i;
            std::vector<uint8_t> in_set(sp.progs.size(), 0), voice_ring(n, 0);
            std::vector<uint32_t> work;
            for (uint32_t i = f0; i < f1; ++i) if (ring_in(need, sp.prog_rings[i])) { in_set[i] = 1; work.push_back(i); }
            for (uint32_t r = 0; r < n; ++r) if (need[r] && bank_ring[r]) voice_ring[r] = 1;
            while (!work.empty()) {
                const StageProg &pg = sp.progs[work.back()];
                work.pop_back();
                for (uint32_t k = 0; k < pg.n_instr; ++k) {
                    const StageInstr &in = sp.instrs[pg.first_instr + k];
                    if (in.op != S_READ && in.op != S_READ_DYN) continue;
                    if (bank_ring[in.buf]) voice_ring[in.buf] = 1;
                    else if (stored_by[in.buf] >= 0 && !in_set[(size_t)stored_by[in.buf]]) { in_set[(size_t)stored_by[in.buf]] = 1; work.push_back((uint32_t)stored_by[in.buf]); }
                }
            }
            add_voices(voice_ring);
            for (uint32_t r = 0; r < n; ++r) if (voice_ring[r]) now[r].valid_from = 0;
            for (size_t l = 0; l + 1 < sp.fused_level_first.size(); ++l) {
                std::vector<std::pair<uint32_t, uint32_t>> runs;
                for (uint32_t i = f0 + sp.fused_level_first[l]; i < f0 + sp.fused_level_first[l + 1]; ++i) {
                    if (!in_set[i]) continue;
                    add_run(runs, i);
                    for (uint32_t r : sp.prog_rings[i]) now[r].valid_from = 0;
                }
                if (!runs.empty()) rp.levels.push_back(std::move(runs));
            }
        }
        ring_state.repair_from = rp.from;
        ring_table.rings = std::move(now);
        ring_table.shard_epoch = shard_epoch;
        return rp;
    }
    std::vector<hipEvent_t> event_pool;
    std::string last_error;
    std::string jit_error;
    std::string plan_json_cache;

    ~fr_renderer() {
        (void)hipSetDevice(device);
        end_stream();
        for (TimerClass *tc : {&t_bank, &t_pull, &t_stage})
            for (auto &pr : tc->pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
        for (Retired &g : graveyard) (void)hipEventDestroy(g.ev);
        if (ev_last) (void)hipEventDestroy(ev_last);
        if (ev_ring_move) (void)hipEventDestroy(ev_ring_move);
        for (hipEvent_t e : x_events) (void)hipEventDestroy(e);
        if (xstream) (void)hipStreamDestroy(xstream);
        // ranges the host registered and never unregistered: the page-lock and the device mapping must not outlive the
        // renderer that made them (the host may free that memory next; a later registration of the same addresses by
        // another renderer would otherwise meet a stale one)
        if (!registered.empty()) (void)hipStreamSynchronize(stream);
        for (auto &rg : registered) { if (hipHostUnregister(rg.first) != hipSuccess) (void)hipGetLastError(); }
        if (host_trace && strm.trace_n)
            std::fprintf(stderr, "fr_stream_block over %llu blocks: ring + wait %.1f us, copy out %.1f us\n", (unsigned long long)strm.trace_n,
                         strm.trace_us[0] / strm.trace_n, strm.trace_us[1] / strm.trace_n);
        if (host_trace && trace_n)
            std::fprintf(stderr, "fr_fill_buffer phases over %llu calls (mapped out %d, mapped in %d): issue %.1f us, %s %.1f us, %s %.1f us\n",
                         (unsigned long long)trace_n, (int)host_out_mapped, (int)host_rows_mapped, trace_us[0] / trace_n,
                         host_out_mapped ? "wait" : "D2H issue", trace_us[1] / trace_n, host_out_mapped ? "CPU copy" : "wait", trace_us[2] / trace_n);
        if (stream) (void)hipStreamDestroy(stream);
    }

    uint64_t implicit_len(uint64_t slot) const {
        for (const Seg &s : segs) if (slot >= s.first && slot < s.last) return s.len;
        return 0;
    }

    // ---- timing ------------------------------------------------------------------------------
    hipEvent_t get_event() {
        if (!event_pool.empty()) { hipEvent_t e = event_pool.back(); event_pool.pop_back(); return e; }
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        return e;
    }
    struct Scope {
        fr_renderer *r; TimerClass *tc; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
        Scope(fr_renderer *rr, TimerClass *t, hipStream_t st) : r(rr), tc(t), s(st) {
            if (r->timing) { a = r->get_event(); b = r->get_event(); HIP_CHECK(hipEventRecord(a, s)); }
        }
        void done() {
            if (a) { HIP_CHECK(hipEventRecord(b, s)); tc->pending.emplace_back(a, b); a = nullptr; }
        }
    };
    void resolve(TimerClass &tc) {
        for (auto &pr : tc.pending) {
            HIP_CHECK(hipEventSynchronize(pr.second));
            float ms = 0;
            HIP_CHECK(hipEventElapsedTime(&ms, pr.first, pr.second));
            tc.ms += ms;
            tc.launches += 1;
            event_pool.push_back(pr.first);
            event_pool.push_back(pr.second);
        }
        tc.pending.clear();
    }

    // ---- observed input ranges (FR_DELAY_OBSERVED, stage.hpp ObservedInputs) ---------------------------------------
    // One hull per input slot of every value stored since the last seek.  It holds +0.0 from the start (unfed slots, zero
    // prefixes and frames beyond what was stored read 0.0), only ever widens until a seek, and a history_frames cap never
    // shrinks it.  Only the slots the plan's observed amounts read are scanned as rows arrive (plan.sp.observed_slots); any
    // other slot that receives data becomes unknown, and is reduced over its stored history when a plan first asks for it.
    bool delay_observed = false;         // FR_DELAY_OBSERVED
    uint64_t delay_observed_max = 1u << 20;   // FR_DELAY_OBSERVED_MAX: the largest look-back the mode plans
    struct Hull {
        float lo = 0.0f, hi = 0.0f;      // finite values
        uint32_t flags = 0;              // kernels.hpp RANGE_*
        bool known = true;
    };
    std::vector<Hull> hulls;
    uint64_t lookback_growths = 0;       // re-plans because stored rows widened an amount's bound past its planned look-back
    uint64_t range_launches = 0;         // input_range_kernel launches
    uint64_t deferred_len = 0;           // frames of every row in `deferred` (the call's n_times)
    PinnedBuf h_range;
    static bool widen(Hull &h, float lo, float hi, uint32_t flags) {
        const bool w = lo < h.lo || hi > h.hi || (flags & ~h.flags) != 0;
        h.lo = std::min(h.lo, lo);
        h.hi = std::max(h.hi, hi);
        h.flags |= flags;
        return w;
    }
    // Reduces device rows with input_range_kernel and waits for the result.  `hull_of[i]` receives row i's values.
    bool reduce_device_rows(const std::vector<std::pair<const float *, uint64_t>> &rows, const std::vector<Hull *> &hull_of, hipStream_t st) {
        bool widened = false;
        for (size_t first = 0; first < rows.size(); first += RANGE_MAX_ROWS) {
            RangeArgs a{};
            a.n_rows = (uint32_t)std::min<size_t>(RANGE_MAX_ROWS, rows.size() - first);
            uint64_t longest = 0;
            for (uint32_t i = 0; i < a.n_rows; ++i) {
                a.row[i] = rows[first + i].first;
                a.len[i] = rows[first + i].second;
                longest = std::max(longest, a.len[i]);
            }
            // (a block per 16 K values: one block covers a real-time call's row, long histories spread over up to 64)
            a.blocks = (uint32_t)std::min<uint64_t>(RANGE_MAX_BLOCKS, std::max<uint64_t>(1, (longest + 16383) / 16384));
            h_range.ensure((size_t)a.n_rows * a.blocks * sizeof(RangePart));
            a.out = h_range.as_dev<RangePart>();
            HIP_CHECK(launch_input_range(a, st));
            ++range_launches;
            HIP_CHECK(hipStreamSynchronize(st));   // the plan depends on the result
            const RangePart *part = h_range.as<RangePart>();
            for (uint32_t i = 0; i < a.n_rows; ++i)
                for (uint32_t b = 0; b < a.blocks; ++b) {
                    const RangePart &o = part[(size_t)i * a.blocks + b];
                    widened = widen(*hull_of[first + i], o.lo, o.hi, o.flags) || widened;
                }
        }
        return widened;
    }
    // The observed range of `slot` for the planner; an unknown hull is first rebuilt from the slot's visible history (plus a
    // row of this call that a bank kernel will append).
    Range observed_range(uint32_t slot, hipStream_t st) {
        // (track slots are never stored, so nothing was observed of them: with a track history their amounts stay unbounded)
        if (tail_on() && slot >= track_from) return Range{-HUGE_VAL, HUGE_VAL, true};
        if (slot >= hulls.size() || slot >= n_vecs) return Range{0.0, 0.0, false};
        Hull &h = hulls[slot];
        if (!h.known) {
            h = Hull{};
            std::vector<std::pair<const float *, uint64_t>> rows;
            const DevInput d = dev_input(slot);
            if (d.data && d.len > d.base) rows.push_back({d.data, d.len - d.base});
            for (const Deferred &df : deferred)
                if (df.slot == slot && df.dst) rows.push_back({df.src, deferred_len});
            reduce_device_rows(rows, std::vector<Hull *>(rows.size(), &h), st);
        }
        return Range{(h.flags & RANGE_NEG_INF) ? -HUGE_VAL : (double)h.lo, (h.flags & RANGE_POS_INF) ? HUGE_VAL : (double)h.hi,
                     (h.flags & RANGE_NAN) != 0};
    }
    ObservedInputs observed_inputs(hipStream_t st) {
        ObservedInputs o;
        o.max_lookback = delay_observed_max;
        o.range = [this, st](uint32_t slot) { return observed_range(slot, st); };
        return o;
    }
    // store_inputs, before any row is stored: takes this call's rows of the observed slots into their hulls, and marks the
    // plan stale when they widen a bound past its planned look-back (the call re-plans, rebuilding the rings' window with
    // the larger look-back) or when a seek lets bounds shrink.  Only plans with observed slots scan; only device rows wait.
    void observe_rows(uint32_t n_slots, uint32_t rows, const float *in_data, const uint64_t *offs, bool device_rows, bool seek, hipStream_t st) {
        if (seek) {
            for (Hull &h : hulls) h = Hull{};
            if (plan.valid && (!plan.sp.observed.empty() || plan.sp.observed_refused)) plan.observed_stale = true;
        }
        if (hulls.size() < rows) hulls.resize(rows);
        const std::vector<uint32_t> &want = plan.sp.observed_slots;   // (the plan in hand: its successor reads the same slots)
        std::vector<std::pair<const float *, uint64_t>> dev_rows;
        std::vector<Hull *> dev_hulls;
        bool widened = false;
        for (uint32_t r = 0; r < rows; ++r) {
            const uint64_t rl = offs[r + 1] - offs[r];
            if (!rl) continue;   // (padding repeats the last stored value, or 0.0: both already in the hull)
            Hull &h = hulls[r];
            if (!h.known || !std::binary_search(want.begin(), want.end(), r)) { h.known = false; continue; }
            if (device_rows) {
                dev_rows.push_back({in_data + offs[r], rl});
                dev_hulls.push_back(&h);
                continue;
            }
            float lo = HUGE_VALF, hi = -HUGE_VALF;
            uint32_t fl = 0;
            for (const float *v = in_data + offs[r], *e = v + rl; v != e; ++v) {
                const float x = *v;
                if (x >= -FLT_MAX && x <= FLT_MAX) { lo = std::min(lo, x); hi = std::max(hi, x); }
                else fl |= x != x ? RANGE_NAN : x > 0.0f ? RANGE_POS_INF : RANGE_NEG_INF;
            }
            widened = widen(h, lo, hi, fl) || widened;
        }
        if (!dev_rows.empty()) widened = reduce_device_rows(dev_rows, dev_hulls, st) || widened;
        if (widened && !seek && plan_current(n_slots) && !plan.sp.observed.empty() && !observed_plan_holds(*plan.graph, plan.sp, observed_inputs(st))) {
            plan.observed_stale = true;
            ++lookback_growths;
        }
    }

    // ---- input store (reference.rs:47-75) -------------------------------------------------------
    // Frames of input history kept per slot (0 = everything since the last seek: the reference, reference.rs:25).  With
    // fr_config.history_frames set, at least what the current plan's constant delays and proven bounds can reach.
    uint64_t keep_frames() const {
        return store_keep_frames(history_frames, plan.valid, plan.sp.input_lookback);
    }
    // Buffers replaced by bigger ones are freed once the stream has passed the copy out of them -- never by waiting.
    uint64_t call_idx = 0;               // first frame of the call being served
    uint64_t history_floor = 0;          // bounded history: input samples before this frame read as 0.0 (monotone)
    struct Retired { DevBuf buf; hipEvent_t ev; };
    std::vector<Retired> graveyard;
    void bury(DevBuf &&b, hipStream_t st) {
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, st) != hipSuccess) {
            (void)hipGetLastError();
            HIP_CHECK(hipStreamSynchronize(st));   // (cannot track it: wait once)
            if (ev) (void)hipEventDestroy(ev);
            return;                                // `b` is freed here
        }
        graveyard.push_back(Retired{std::move(b), ev});
    }
    void reap() {
        for (size_t i = 0; i < graveyard.size();) {
            if (hipEventQuery(graveyard[i].ev) == hipSuccess) {
                (void)hipEventDestroy(graveyard[i].ev);
                graveyard[i] = std::move(graveyard.back());
                graveyard.pop_back();
            } else {
                (void)hipGetLastError();
                ++i;
            }
        }
    }
    // Room for n_times more frames in slot s.  Bounded history slides in place (the newest `keep` frames move to the
    // front of a buffer sized 2 * (keep + call) -- one small device copy every `keep` frames, no allocation); unbounded
    // history doubles into a new buffer with an asynchronous copy, the old buffer retired without a stream wait.
    void make_room(InSlot &s, uint64_t n_times, hipStream_t st) {
        // (which of the three it is: streamstore.hpp store_room, the rule a stream that stores its rows asks before every block)
        const uint64_t stored = s.len - s.base;
        const StoreRoom room = store_room(stored, s.cap, keep_frames(), n_times);
        if (room.kind == StoreRoom::fits) return;
        if (last_pending) HIP_CHECK(hipDeviceSynchronize());   // a call on another stream may still be appending to this buffer
        if (room.kind == StoreRoom::slide) {                    // source and destination do not overlap
            HIP_CHECK(hipMemcpyAsync(s.buf.p, s.buf.as<float>() + room.drop, room.kept * sizeof(float), hipMemcpyDeviceToDevice, st));
            s.base += room.drop;
            return;
        }
        DevBuf nb;
        nb.ensure(room.cap * sizeof(float));
        if (room.kept) HIP_CHECK(hipMemcpyAsync(nb.p, s.buf.as<float>() + room.drop, room.kept * sizeof(float), hipMemcpyDeviceToDevice, st));
        s.base += room.drop;
        if (s.buf.p) bury(std::move(s.buf), st);
        s.buf = std::move(nb);
        s.cap = room.cap;
    }

    // A full-length device-resident row feeding a bank's time slot is not copied here: the bank kernel reads
    // the caller's row directly and appends it to the history itself (BankArgs::hist_dst).
    // (`appended_tile`: the exchange-window tile whose launch last appended its part of the row, by offset; -1: none has)
    struct Deferred { uint32_t slot; const float *src; float *dst; int64_t appended_tile = -1; };
    std::vector<Deferred> deferred;
    // Will execute() render exactly [idx, idx + n_times) for the staged part (steady state), or rebuild a look-back
    // window first?  Same conditions as execute() uses (ring capacity, contiguity with what the rings hold).
    // (FR_RING_KEEP: conservative.  The first call of a new plan answers "not steady" here even when execute() then keeps every
    //  ring and runs the call in its steady form: whether it repairs is known only once the rings are matched, and a repair
    //  reads the stored history.  The row is then stored ahead and nothing is deferred -- one row copy, once per re-plan.)
    bool steady_call(uint64_t idx, uint64_t n_times) const {
        const StagedPlan &sp = plan.sp;
        if (!sp.uses_rings()) return true;
        uint64_t need = sp.lmax + n_times, cap = 1024;
        while (cap < need) cap <<= 1;
        if (cap > ring_cap || (size_t)sp.n_rings * ring_cap * sizeof(float) > d_rings.bytes) return false;
        return plan.stage_valid && plan.stage_end == idx;
    }
    bool bank_time_slot(uint32_t n_slots, uint64_t n_times, uint32_t slot, uint64_t idx) const {
        if (!plan_current(n_slots)) return false;
        // a window with look-back reads the stored history, so the row must be there first; in steady state the bank
        // launch (always ahead of the programs on the stream) reads the caller's row and appends it like any other
        if ((plan.sp.uses_rings() || !plan.sp.progs.empty()) && !steady_call(idx, n_times)) return false;
        bool any = false;
        for (const BankStage &bs : plan.banks) {
            const std::vector<uint32_t> &in = bs.grp.shape.input_slots;
            if (bs.grp.jit ? std::find(in.begin(), in.end(), slot) == in.end() : bs.grp.input_slot != slot) continue;
            // only a launch that appends history may take the row: not the compiled or schedule kernels, nor bank_small_kernel
            // (row flags do not change that answer)
            if (!plan_bank_launch(bs, n_times, false).appends_rows) return false;
            any = true;
        }
        return any;
    }

    // What a failed call must put back: the input store is committed before the kernels run, and execute() can still
    // fail (device errors, out of memory).  Without a seek the slots' lengths, the implicit segments and the vec count
    // go back to what they were; after a seek the old samples may already be overwritten, so the store stays in the
    // state the seek itself produces (everything zero before idx) -- the retry at the same idx seeks again anyway.
    struct StoreSnapshot {
        struct S { bool fed; uint64_t base, len; };
        std::vector<S> slots;
        std::vector<Seg> segs;
        uint64_t n_vecs = 0;
        bool seeked = false;
        uint64_t idx = 0;
    };
    StoreSnapshot snapshot_store(uint64_t idx) const {
        StoreSnapshot sn;
        sn.slots.reserve(slots.size());
        for (const InSlot &s : slots) sn.slots.push_back({s.fed, s.base, s.len});
        sn.segs = segs;
        sn.n_vecs = n_vecs;
        sn.seeked = idx != head;
        sn.idx = idx;
        return sn;
    }
    void rollback_store(const StoreSnapshot &sn) {
        deferred.clear();
        plan.stage_valid = false;   // rings may hold part of the failed call's window
        if (rings_touched) ring_table.valid = false;   // (a call refused before it launched anything left the rings as they were)
        counters_dirty = true;      // a launch of the failed call may have stopped half-way through its tickets / row counts
        if (sn.seeked) {
            for (InSlot &s : slots) { s.base = sn.idx; s.len = sn.idx; }
            return;
        }
        for (size_t i = 0; i < slots.size(); ++i) {
            if (i < sn.slots.size()) {
                // (a bounded history may have slid forward meanwhile: the buffer then starts at the later base)
                slots[i].fed = sn.slots[i].fed;
                slots[i].base = std::min(std::max(slots[i].base, sn.slots[i].base), sn.slots[i].len);
                slots[i].len = sn.slots[i].len;
            }
            else { slots[i].fed = false; slots[i].base = slots[i].len = 0; }
        }
        segs = sn.segs;
        n_vecs = sn.n_vecs;
    }

    // `device_rows`: in_data is a device pointer (fr_fill_buffer_device).
    // `dense`: the rows are an [n_rows][n_times] matrix (fr_fill_buffer_dense); `offs` then covers the stored rows only.
    void store_inputs(uint32_t n_slots, uint64_t n_times, uint64_t idx, const float *in_data,
                      const uint64_t *offs, uint32_t n_rows, bool device_rows, hipStream_t st, bool dense = false) {
        deferred.clear();
        track_dev.clear();
        reap();
        rings_touched = false;
        call_idx = idx;
        call_tracks = nullptr;
        call_track_stride = call_track_rows = 0;
        if (dense_total_rows) { dense = true; n_rows = dense_total_rows; }   // (fr_fill_buffer_dense: `offs` covers min(rows, track_from) rows)
        {   // rows beyond the reference's input vectors -- n_slots * n_times of the largest call so far -- are dropped (reference.rs:59-68)
            const uint64_t vecs_after = std::max<uint64_t>(n_vecs, (uint64_t)n_slots * n_times);
            if (track_from != 0xFFFFFFFFu && n_rows > vecs_after) n_rows = (uint32_t)vecs_after;
        }
        if (n_rows > track_from && n_times > 0) {   // rows of track slots: not stored, read in place by this call's voices
            if (!dense)
                for (uint32_t r = track_from; r < n_rows; ++r)
                    if (offs[r + 1] - offs[r] != n_times)
                        throw Error(FR_ERR_UNSUPPORTED, "track input row " + std::to_string(r) + " must hold exactly the " + std::to_string(n_times) + " frames rendered");
            const float *first = in_data + (dense ? (uint64_t)track_from * n_times : offs[track_from]);
            const uint64_t rows_t = n_rows - track_from;
            if (!device_rows) {
                d_tracks_stage.ensure(rows_t * n_times * sizeof(float));
                HIP_CHECK(hipMemcpyAsync(d_tracks_stage.p, first, rows_t * n_times * sizeof(float), hipMemcpyHostToDevice, st));
                first = d_tracks_stage.as<float>();
            }
            call_tracks = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(first) - (uintptr_t)track_from * n_times * sizeof(float));
            call_track_stride = n_times;
            call_track_rows = rows_t;
            n_rows = track_from;
        } else if (dense_total_rows) {
            n_rows = std::min(n_rows, track_from);
        }
        const bool seek = idx != head;   // forget history, act as if inputs were 0 before idx (renderer.rs:12-15)
        // validate everything before mutating so a refused call leaves the history intact: the lengths the rows must
        // continue are those AFTER the seek (idx for every vec) and after the vec count grew (reference.rs:52-71)
        {
            const uint64_t want = (uint64_t)n_slots * n_times;
            const uint64_t vecs_after = std::max(n_vecs, want);
            const uint32_t rows = (uint32_t)std::min<uint64_t>(n_rows, vecs_after);
            for (uint32_t r = 0; r < rows; ++r) {
                uint64_t cur = idx;   // after a seek, and for vecs created by this call
                if (!seek && r < n_vecs) cur = (r < slots.size() && slots[r].fed) ? slots[r].len : implicit_len(r);
                if (cur != idx)
                    throw Error(FR_ERR_INPUT_HISTORY, "input slot " + std::to_string(r) + " holds " + std::to_string(cur) +
                                                          " samples, expected idx=" + std::to_string(idx));
                if (offs[r + 1] < offs[r] || offs[r + 1] - offs[r] > n_times)
                    throw Error(FR_ERR_INPUT_TOO_LONG, "input row " + std::to_string(r) + " longer than the range rendered");
            }
        }
        if (seek) {
            for (InSlot &s : slots) { s.base = idx; s.len = idx; }
            segs.clear();
            if (n_vecs) segs.push_back({0, n_vecs, idx});
            history_floor = 0;   // (everything before idx is zero now anyway)
        }
        {   // bounded history: what this call may see, and no later call may see more (deterministic whatever slack the
            // buffers happen to hold when a longer Delay arrives)
            history_floor = store_floor(history_floor, keep_frames(), idx);
        }
        uint64_t want = (uint64_t)n_slots * n_times;   // `buff.len()`, reference.rs:60 (element count, a quirk)
        if (n_vecs < want) { segs.push_back({n_vecs, want, idx}); n_vecs = want; }
        uint32_t rows = (uint32_t)std::min<uint64_t>(n_rows, n_vecs);   // zip stops at the shorter (:68)
        if (rows > slots.size()) slots.resize(rows);
        deferred_len = n_times;
        if (delay_observed) observe_rows(n_slots, rows, in_data, offs, device_rows, seek, st);
        // (every host-buffer call ends with a stream synchronisation, so the staging buffer is idle here)
        if (!device_rows && rows) h_in_stage.ensure((size_t)rows * n_times * sizeof(float));
        for (uint32_t r = 0; r < rows; ++r) {
            InSlot &s = slots[r];
            if (!s.fed) { s.fed = true; s.base = implicit_len(r); s.len = s.base; }
            uint64_t rl = offs[r + 1] - offs[r];
            uint64_t stored = s.len - s.base;
            make_room(s, n_times, st);
            stored = s.len - s.base;
            float *dst = s.buf.as<float>() + stored;
            if (device_rows && rl == n_times && rl > 0 && bank_time_slot(n_slots, n_times, r, idx)) {
                deferred.push_back(Deferred{r, in_data + offs[r], dst});
            } else if (device_rows) {
                if (rl) HIP_CHECK(hipMemcpyAsync(dst, in_data + offs[r], rl * sizeof(float), hipMemcpyDeviceToDevice, st));
                if (rl < n_times) {
                    // pad with the last value now stored, or 0 (reference.rs:72-73)
                    const float *last = (stored + rl) ? dst + rl - 1 : nullptr;
                    HIP_CHECK(launch_pad(dst + rl, n_times - rl, last, st));
                }
            } else {
                // host rows: row + padding assembled in this row's region of the pinned staging buffer, one H2D copy,
                // no sync (the region is not touched again before the call's final synchronisation)
                float pad = 0.0f;
                if (rl) pad = in_data[offs[r] + rl - 1];
                else if (stored) {
                    HIP_CHECK(hipMemcpyAsync(&pad, dst - 1, sizeof(float), hipMemcpyDeviceToHost, st));
                    HIP_CHECK(hipStreamSynchronize(st));
                }
                float *stage = h_in_stage.as<float>() + (size_t)r * n_times;
                if (rl) std::memcpy(stage, in_data + offs[r], rl * sizeof(float));
                std::fill(stage + rl, stage + n_times, pad);
                if (host_rows_mapped && n_times > 0 && bank_time_slot(n_slots, n_times, r, idx)) {
                    // no copy at all: the bank kernel reads the row through the mapping and appends it to the history in
                    // HBM itself (as it does for device-resident rows)
                    deferred.push_back(Deferred{r, h_in_stage.as_dev<float>() + (size_t)r * n_times, dst});
                } else {
                    HIP_CHECK(hipMemcpyAsync(dst, stage, n_times * sizeof(float), hipMemcpyHostToDevice, st));
                }
            }
            s.len += n_times;
        }
    }

    DevInput dev_input(uint32_t slot) const {
        DevInput d{nullptr, 0, 0};
        if (slot >= track_from && !track_dev.empty()) {   // a track read through an input table (track history)
            auto it = std::lower_bound(track_dev.begin(), track_dev.end(), std::make_pair(slot, d),
                                       [](const std::pair<uint32_t, DevInput> &x, const std::pair<uint32_t, DevInput> &y) { return x.first < y.first; });
            return it != track_dev.end() && it->first == slot ? it->second : d;
        }
        if (slot < slots.size() && slots[slot].fed && slot < n_vecs) {
            const InSlot &s = slots[slot];
            d.data = s.buf.as<float>();
            d.base = s.base;
            d.len = s.len;
            // bounded history: exactly `keep` frames before the call's first frame are visible, whatever slack the
            // buffer still holds (so that results do not depend on when the buffer last slid)
            if (history_floor > d.base) {
                const uint64_t floor = std::min(history_floor, d.len);
                d.data += floor - d.base;
                d.base = floor;
            }
        }
        return d;
    }
    // A slot's stored history over the window [b0, b0 + len) (BankArgs::time, JitBankArgs::in): `data` holds window frame
    // `skip` onwards, `valid` frames of it; zero before the stored history (seek) and beyond it.  Untouched without history.
    template <class U>
    void input_window(uint32_t slot, uint64_t b0, uint64_t len, const float *&data, U &skip, U &valid) const {
        const DevInput d = dev_input(slot);
        if (!d.data || d.len <= d.base) return;
        const uint64_t start = std::max(b0, d.base);
        skip = std::min(start - b0, len);
        data = d.data + (start - d.base);
        valid = d.len > start ? d.len - start : 0;
    }

    // ---- planning ---------------------------------------------------------------------------------
    void build_plan(uint32_t n_slots, hipStream_t st) {
        Plan p;
        p.version = mirror.version;
        p.shard_epoch = shard_epoch;
        p.n_slots = n_slots;
        const ShardSpec *shard_spec = sharded() ? &shard : nullptr;
        const auto t_begin = std::chrono::steady_clock::now();
        // a rank of a voice-sharded job lowers only the rows it owns (1/world of the first-call cost; graph errors on another
        // rank's rows are that rank's to report); partial-block sharding analyses the whole graph on every rank
        uint32_t lower_lo = 0, lower_hi = UINT32_MAX;
        if (sharded() && shard.mode == FR_SHARD_VOICES) my_rows(n_slots, lower_lo, lower_hi);
        // (partial-block sharding: every rank must arrive at the same node ids -- the exchange is ordered by them)
        lowering.set_loop_dyn(loop_dyn != 0);
        const FlatGraph &fg = lowering.update(mirror, n_slots, lower_lo, lower_hi, sharded() && shard.mode == FR_SHARD_PARTIALS);
        const double lower_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        p.max_depth = fg.max_depth;
        bool use_jit = allow_jit && mode == FR_MODE_AUTO;
        if (!matcher || matcher_gen != lowering.generation()) {
            matcher.reset(new BankMatcher(fg, 20, use_jit, allow_template, track_from));
            matcher_gen = lowering.generation();
        }
        p.graph = &fg;
        const ObservedInputs obs = observed_inputs(st);
        const ObservedInputs *observed = delay_observed ? &obs : nullptr;
        p.sp = plan_stages(fg, mode == FR_MODE_AUTO, mode != FR_MODE_PULL, 20, use_jit, allow_template, matcher.get(), shard_spec, track_from, observed, track_history, loop_tiles, loop_dyn != 0);
        renumber_rings(p.sp);
        std::vector<std::shared_ptr<JitKernel>> jits(p.sp.banks.size());
        p.jit_epoch = jit_cache.epoch();   // (read first: a compile finishing from here on makes this plan stale)
        if (use_jit) {
            bool without = false;
            try {
                for (size_t i = 0; i < p.sp.banks.size(); ++i)
                    if (p.sp.banks[i].jit) {
                        // (voices that read tracks have no other evaluator to render with meanwhile: wait for the compiler)
                        const bool wait = p.sp.banks[i].tracks && jit_async_configured;
                        if (wait) jit_cache.set_async(false);
                        struct Restore { JitCache &c; bool on; ~Restore() { if (on) c.set_async(true); } } restore{jit_cache, wait};
                        jits[i] = jit_cache.get(p.sp.banks[i].shape, p.sp.banks[i].varying, p.sp.banks[i].literal_bits, p.sp.banks[i].alias);
                        if (!jits[i]) p.jit_pending = without = true;   // being compiled on the worker thread: do not wait
                    }
            } catch (const Error &e) {   // hipRTC unavailable or the generated source did not compile: plan without it
                jit_error = e.what();
                without = true;
                // ... unless the plan must be the SAME on every rank (partial-block sharding: the list of split voices is the
                // exchange's schedule): a rank that re-planned on its own would send ranges its peers do not expect, and the
                // job would hang in the transport.  There the failure is the call's.  (FR_ERR_UNSUPPORTED = no run-time compiler in
                // this build at all -- the same on every rank of it, so planning without is still planning alike.)
                if (sharded() && shard.mode == FR_SHARD_PARTIALS && e.code != FR_ERR_UNSUPPORTED)
                    throw Error(FR_ERR_DEVICE, std::string("a kernel of the sharded plan could not be compiled on this rank (every rank must plan alike): ") + e.what());
            }
            if (without) {
                p.sp = plan_stages(fg, true, true, 20, false, true, nullptr, shard_spec, track_from, observed, track_history, loop_tiles, loop_dyn != 0);
                renumber_rings(p.sp);
                jits.assign(p.sp.banks.size(), nullptr);
            }
        }
        size_t bank_i = 0;
        for (BankLaunch &bg : p.sp.banks) {
            BankStage bs;
            bs.jit = jits[bank_i++];
            bs.grp = std::move(bg);
            bs.d_params.ensure(bs.grp.params.size() * sizeof(float));
            bs.d_rows.ensure(bs.grp.rows.size() * sizeof(uint32_t));
            HIP_CHECK(hipMemcpyAsync(bs.d_params.p, bs.grp.params.data(), bs.grp.params.size() * sizeof(float), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(bs.d_rows.p, bs.grp.rows.data(), bs.grp.rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            if (bs.grp.general) {
                bs.d_groups.ensure(bs.grp.groups.size() * sizeof(uint32_t));
                bs.d_group_off.ensure(bs.grp.group_off.size() * sizeof(uint32_t));
                HIP_CHECK(hipMemcpyAsync(bs.d_groups.p, bs.grp.groups.data(), bs.grp.groups.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
                HIP_CHECK(hipMemcpyAsync(bs.d_group_off.p, bs.grp.group_off.data(), bs.grp.group_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            }
            p.banks.push_back(std::move(bs));
        }
        p.sp.banks.clear();
        if (!p.sp.split.empty()) {
            std::vector<uint32_t> dst(p.sp.split.size());
            for (size_t i = 0; i < dst.size(); ++i) dst[i] = p.sp.split[i].dst | (p.sp.split[i].to_ring ? 0x80000000u : 0u);
            p.d_split_dst.ensure(dst.size() * sizeof(uint32_t));
            HIP_CHECK(hipMemcpyAsync(p.d_split_dst.p, dst.data(), dst.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));   // `dst` goes out of scope
        }
        if (!p.sp.progs.empty()) {
            p.d_instrs.ensure(p.sp.instrs.size() * sizeof(StageInstr));
            p.d_progs.ensure(p.sp.progs.size() * sizeof(StageProg));
            HIP_CHECK(hipMemcpyAsync(p.d_instrs.p, p.sp.instrs.data(), p.sp.instrs.size() * sizeof(StageInstr), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(p.d_progs.p, p.sp.progs.data(), p.sp.progs.size() * sizeof(StageProg), hipMemcpyHostToDevice, st));
            StageJitPlan sj;
            p.loop_tile = loop_tile(p.sp, loop_tiles);
            p.loop_sweep = loop_sweep(p.sp, loop_dyn);
            // (a sweep plan runs on the interpreter: there are no generated sweep programs)
            if (allow_jit && stage_jit_mode != 0 && !p.sp.fused_sweep && plan_stage_jit(p.sp.progs, p.sp.instrs, 32, stage_jit_mode == 2, sj, mirror.sparkle,
                                                                              stage_block_env ? stage_block_env : (p.sp.feedback ? 16u : 1u),
                                                                              p.sp.feedback && p.sp.fused_carry_only, p.loop_tile.frames)) {
                try {
                    p.stage_jit = jit_cache.get_source(sj.source, "jit_stage");
                    if (!p.stage_jit) {   // still compiling: the interpreter serves the calls until the plan is rebuilt
                        p.jit_pending = true;
                        throw Error(FR_OK, "");
                    }
                    p.stage_shapes = sj.n_shapes;
                    p.stage_jit_form.deep = sj.deep;
                    p.stage_jit_form.defer = sj.defer;
                    p.stage_jit_form.maxp = sj.maxp;
                    p.stage_jit_form.maxld = sj.maxld;
                    p.stage_jit_form.maxst = sj.maxst;
                    p.stage_jit_form.blk = sj.blk;
                    p.stage_jit_form.tile = sj.tile;
                    p.d_jprogs.ensure(sj.progs.size() * sizeof(JitStageProg));
                    p.d_ptab.ensure(std::max<size_t>(sj.ptab.size(), 1) * sizeof(uint32_t));
                    HIP_CHECK(hipMemcpyAsync(p.d_jprogs.p, sj.progs.data(), sj.progs.size() * sizeof(JitStageProg), hipMemcpyHostToDevice, st));
                    if (!sj.ptab.empty())
                        HIP_CHECK(hipMemcpyAsync(p.d_ptab.p, sj.ptab.data(), sj.ptab.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
                    HIP_CHECK(hipStreamSynchronize(st));   // `sj` goes out of scope
                } catch (const Error &e) {   // keep the interpreter
                    if (e.code != FR_OK) jit_error = e.what();
                    p.stage_jit = nullptr;
                }
            }
        }
        p.pull_rows = p.sp.pull_rows;
        if (!p.pull_rows.empty()) {
            // dense input table: OP_INPUT.a becomes an index into input_slots
            std::vector<DevNode> dn(fg.nodes.size());
            std::unordered_map<uint32_t, uint32_t> dense;
            for (size_t i = 0; i < dn.size(); ++i) {
                const FlatNode &n = fg.nodes[i];
                dn[i] = DevNode{n.op, n.a, n.b, n.depth};
                if (n.op == OP_INPUT) {
                    auto it = dense.emplace(n.a, (uint32_t)p.input_slots.size());
                    if (it.second) p.input_slots.push_back(n.a);
                    dn[i].a = it.first->second;
                }
            }
            std::vector<uint32_t> roots(n_slots);
            for (uint32_t r = 0; r < n_slots; ++r) roots[r] = fg.outputs[r];
            p.d_nodes.ensure(dn.size() * sizeof(DevNode));
            p.d_roots.ensure(roots.size() * sizeof(uint32_t));
            HIP_CHECK(hipMemcpyAsync(p.d_nodes.p, dn.data(), dn.size() * sizeof(DevNode), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipMemcpyAsync(p.d_roots.p, roots.data(), roots.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));   // host vectors above go out of scope
        // description
        std::ostringstream js;
        js << "{\"backend\":\"hip-gfx950\",\"mode\":" << mode << ",\"n_slots\":" << n_slots
           << ",\"lowered_nodes\":" << fg.nodes.size() << ",\"max_depth\":" << fg.max_depth
           << ",\"lowering\":\"" << (lowering.last_was_full() ? "full" : "incremental") << "\",\"relowered_nodes\":" << lowering.last_relowered()
           << ",\"lower_ms\":" << lower_ms << ",\"plans_built\":" << plans_built + 1 << ",\"banks\":[";
        for (size_t i = 0; i < p.banks.size(); ++i) {
            const BankLaunch &g = p.banks[i].grp;
            js << (i ? "," : "") << "{\"voices\":" << g.rows.size() << ",\"partials\":" << (g.general ? g.max_leaves : (1u << g.log2_p))
               << ",\"general_tree\":" << (g.general ? "true" : "false") << ",\"jit\":" << (g.jit ? "true" : "false")
               << ",\"leaf_ops\":" << (g.jit ? g.shape.ops.size() : 0) << ",\"leaf_params\":" << (g.jit ? g.k : 2)
               << ",\"input_slot\":" << g.input_slot << ",\"fast_ok\":" << (g.fast_ok ? "true" : "false")
               << ",\"to_ring\":" << (g.to_ring ? "true" : "false") << ",\"to_exchange\":" << (g.to_ws ? "true" : "false")
               << ",\"tracks\":" << (g.tracks ? "true" : "false")
               << ",\"param_bytes\":" << g.params.size() * sizeof(float) << "}";
        }
        js << "],\"stage_programs\":" << (p.sp.progs.size() - p.sp.fused_count - p.sp.post_count) << ",\"stage_instrs\":" << p.sp.instrs.size()
           << ",\"fused_programs\":" << p.sp.fused_count << ",\"fused_max_frames\":" << p.sp.fused_max_frames << ",\"fused_stride\":" << p.sp.fused_stride
           << ",\"feedback\":" << (p.sp.feedback ? "true" : "false") << ",\"feedback_loops\":" << p.sp.feedback_loops
           << ",\"fused_levels\":" << (p.sp.fused_level_first.empty() ? 0 : p.sp.fused_level_first.size() - 1) << ",\"copy_programs\":" << p.sp.post_count
           << ",\"stage_levels\":" << (p.sp.level_first.empty() ? 0 : p.sp.level_first.size() - 1)
           << ",\"stage_jit\":" << (p.stage_jit ? "true" : "false") << ",\"stage_shapes\":" << p.stage_shapes
           << ",\"stage_jit_form\":" << stage_jit_form_json(p, loop_tiles_given)
           << ",\"fused_carry_only\":" << (p.sp.feedback && p.sp.fused_carry_only ? "true" : "false")
           << ",\"stage_hoisted_max\":" << stage_hoisted_max(p.sp)
           << ",\"rings\":" << p.sp.n_rings << ",\"max_lookback\":" << p.sp.lmax
           << ",\"input_lookback\":" << p.sp.input_lookback << ",\"input_lookback_unbounded\":" << (p.sp.input_lookback_unbounded ? "true" : "false")
           << ",\"delay_observed\":" << (delay_observed ? "true" : "false") << ",\"delay_observed_max\":" << delay_observed_max
           << ",\"observed_delays\":" << p.sp.observed.size() << ",\"observed_lookback\":" << p.sp.observed_lookback
           << ",\"observed_refused\":" << p.sp.observed_refused
           << ",\"history_frames\":" << history_frames << ",\"ring_keep\":" << (ring_keep ? "true" : "false");
        if (loop_tiles_given)
            js << ",\"loop_tiles\":{\"frames\":" << p.loop_tile.frames << ",\"max_stride\":" << LOOP_TILE_MAX_STRIDE << ",\"reason\":\""
               << p.loop_tile.reason << "\"}";
        if (loop_dyn_given)
            js << ",\"loop_dyn\":{\"sweep\":" << p.loop_sweep.sweep << ",\"frames\":" << p.loop_sweep.frames << ",\"form\":\"" << p.loop_sweep.form_name()
               << "\",\"reason\":\"" << p.loop_sweep.reason << "\"}";
        js
           << ",\"track_history\":" << track_history << ",\"track_lookback\":" << p.sp.track_lookback
           << ",\"track_window_slots\":" << p.sp.track_window_slots.size()
           << ",\"jit_pending\":" << (p.jit_pending ? "true" : "false") << ",\"jit_kernels_compiled\":" << jit_cache.compiled() << ",\"jit_compile_ms\":" << jit_cache.compile_ms() << ",\"jit_disk_hits\":" << jit_cache.disk_hits()
           << ",\"pull_rows\":" << p.pull_rows.size()
           << ",\"shard\":{\"rank\":" << shard.rank << ",\"world\":" << shard.world << ",\"mode\":" << (sharded() ? shard.mode : 0)
           << ",\"split_voices\":" << p.sp.split.size() << ",\"transport\":\"" << (rccl ? "rccl" : has_host_comm ? "host-callback" : "none") << "\"}"
           << ",\"exchange\":{\"max_tiles\":" << ((shard_flags & FR_SHARD_SERIAL_EXCHANGE) ? 1u : x_max_tiles) << ",\"min_tile_frames\":" << x_min_tile
           << "}"
           << ",\"build_ms\":" << std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count() << "}";
        ++plans_built;
        p.json = js.str();
        p.valid = true;
        plan = std::move(p);
    }

    void ensure_plan(uint32_t n_slots, hipStream_t st) {
        if (!plan_current(n_slots)) build_plan(n_slots, st);
    }

    // ---- track history (FR_TRACK_HISTORY) ------------------------------------------------------------
    // Before the call's readers: a call that does not continue the ring's frames seeks (every frame before idx reads +0.0);
    // rows the call supplies beyond the ring's are added as zeros; the slots read through an input table get their DevInput --
    // the call's rows in place when nothing reads before idx, else their window gathered from the ring and the call's rows.
    void prepare_tracks(uint64_t n_times, uint64_t idx, hipStream_t st) {
        track_dev.clear();
        if (!tail_on()) return;
        if (call_track_rows > tail_rows) {
            DevBuf nb;
            nb.ensure(call_track_rows * tail_cap * sizeof(float));
            HIP_CHECK(hipMemsetAsync(nb.p, 0, call_track_rows * tail_cap * sizeof(float), st));
            if (tail_rows && tail_end == idx) HIP_CHECK(hipMemcpyAsync(nb.p, d_tail.p, tail_rows * tail_cap * sizeof(float), hipMemcpyDeviceToDevice, st));
            if (d_tail.p) bury(std::move(d_tail), st);
            d_tail = std::move(nb);
            tail_rows = (uint32_t)call_track_rows;
            tail_end = idx;
        }
        if (tail_end != idx) {
            if (tail_rows) HIP_CHECK(hipMemsetAsync(d_tail.p, 0, tail_rows * tail_cap * sizeof(float), st));
            tail_end = idx;
        }
        const std::vector<uint32_t> &slots = plan.sp.track_window_slots;
        if (slots.empty()) return;
        const uint64_t back = std::min(idx, plan.sp.track_lookback);
        auto call_row = [&](uint32_t sl) -> const float * {
            return call_tracks && sl - track_from < call_track_rows ? call_tracks + (uint64_t)sl * call_track_stride : nullptr;
        };
        if (back == 0) {
            for (uint32_t sl : slots) {
                const float *row = call_row(sl);
                track_dev.push_back({sl, row ? DevInput{row, idx, idx + n_times} : DevInput{nullptr, 0, 0}});
            }
            return;
        }
        const uint64_t len = back + n_times;
        used_scratch = true;
        d_track_win.ensure(slots.size() * len * sizeof(float));
        TrackWindowArgs a{};
        a.mask = tail_cap - 1;
        a.idx = idx;
        a.back = back;
        a.n = n_times;
        for (size_t i = 0; i < slots.size(); ++i) {
            float *dst = d_track_win.as<float>() + i * len;
            const uint32_t row = slots[i] - track_from;
            a.dst[a.n_rows] = dst;
            a.tail[a.n_rows] = row < tail_rows ? d_tail.as<float>() + (uint64_t)row * tail_cap : nullptr;
            a.call[a.n_rows] = call_row(slots[i]);
            if (++a.n_rows == TRACK_WINDOW_MAX_ROWS || i + 1 == slots.size()) {
                HIP_CHECK(launch_track_window(a, st));
                a.n_rows = 0;
            }
            track_dev.push_back({slots[i], DevInput{dst, idx - back, idx + n_times}});
        }
    }
    // After every reader of the call: its last min(n, ring) columns of every track row into the ring (rows it did not supply,
    // or that the buff.len() limit dropped, as +0.0).
    void append_tracks(uint64_t n_times, uint64_t idx, hipStream_t st) {
        tail_launches = 0;
        if (!tail_on() || n_times == 0) return;
        track_dev.clear();
        used_scratch = true;
        if (tail_rows) {
            TrackTailArgs a{};
            a.tail = d_tail.as<float>();
            a.src = call_tracks ? call_tracks + (uint64_t)track_from * call_track_stride : nullptr;
            a.src_stride = call_track_stride;
            a.src_rows = call_tracks ? (uint32_t)std::min<uint64_t>(call_track_rows, tail_rows) : 0;
            a.rows = tail_rows;
            a.mask = tail_cap - 1;
            a.count = std::min(n_times, tail_cap);
            a.col0 = n_times - a.count;
            a.first = idx + a.col0;
            Scope sc(this, &t_stage, st);
            HIP_CHECK(launch_track_tail(a, st));
            sc.done();
            ++tail_launches;
        }
        tail_end = idx + n_times;
    }

    // ---- execution --------------------------------------------------------------------------------
    // One render call, as its phases see it: the destination, the call itself (callplan.hpp CallIn, filled in by
    // prepare_rings) and what the per-call rule answered for it.
    struct Call : CallIn {
        float *dst;
        uint32_t n_slots;
        hipStream_t st;
        Call(float *d, uint32_t slots, uint64_t n, uint64_t first, hipStream_t s) : dst(d), n_slots(slots), st(s) { idx = first; n_times = n; }
        CallWindows w;
        ExchangeTiles xt;
        StageForm form;
        bool x_window_is_call() const { return w.x0 == idx && w.xlen == n_times; }
        bool pipelined() const { return xt.count > 1; }   // the tiles' exchanges run on the exchange stream, under later tiles' kernels
    };

    void execute(float *d_dst, uint32_t n_slots, uint64_t n_times, uint64_t idx, hipStream_t st) {
        bank_launches.clear();
        stage_launches.clear();
        bank_form = "call";
        ensure_plan(n_slots, st);
        rings_touched = true;
        prepare_tracks(n_times, idx, st);
        if (n_slots != 0 && n_times != 0) {   // (nothing to render: the track history still moves on as the reference's inputs do)
            const StagedPlan &sp = plan.sp;
            Call c(d_dst, n_slots, n_times, idx, st);
            const RingRepair repair = prepare_rings(c);
            // (decided AFTER the rings may have been re-allocated above: a longer call than any before loses what they held)
            c.w = call_windows(sp, c);
            const bool serial = exchange_serial((shard_flags & FR_SHARD_SERIAL_EXCHANGE) != 0, rccl != nullptr, x_tiles_explicit);
            if (!sp.split.empty()) c.xt = fr::exchange_tiles(c.w.xlen, serial, x_max_tiles, x_min_tile);
            c.form = stage_form(sp, c, c.w, STRIDED_MIN_STRIDE, fused_strided_ok);
            repair_rings(c, repair);
            replay_feedback(c);
            exchange_split_voices(c);
            launch_whole_banks(c);
            launch_stage_programs(c);
            commit_rings(c);
            if (!plan.pull_rows.empty()) run_pull(d_dst, n_slots, n_times, idx, st);
        }
        append_tracks(n_times, idx, st);
    }

    // A call of ZERO own frames at idx (callplan.hpp bring_up_form): the rings are brought up to idx as the first fr_fill_buffer
    // call of the plan at idx would bring them before its own frames, sized for calls of `ring_frames` frames -- nothing when they
    // are current, the look-back rebuild from the STORED history, a feedback plan's replay, FR_RING_KEEP's keep-and-repair.  A
    // stream that continues the input store (FR_STREAM_STORE) starts its resident launch behind it.  The phases are execute()'s.
    void bring_up_rings(uint32_t n_slots, uint64_t idx, uint64_t ring_frames, hipStream_t st) {
        bank_launches.clear();
        stage_launches.clear();
        bank_form = "call";
        deferred.clear();
        track_dev.clear();
        reap();
        call_idx = idx;
        ensure_plan(n_slots, st);
        rings_touched = true;
        const StagedPlan &sp = plan.sp;
        Call c(nullptr, n_slots, 0, idx, st);
        try {
            const RingRepair repair = prepare_rings(c, ring_frames);
            c.w = call_windows(sp, c);
            c.form = bring_up_form(sp, c, c.w);
            repair_rings(c, repair);
            replay_feedback(c);
            if (c.w.w_len != 0)
                for (BankStage &bs : plan.banks)
                    if (bs.grp.to_ring) launch_bank_window(c, bs, c.w.w0, c.w.w_len, -1);
            launch_stage_programs(c);
            commit_rings(c);
        } catch (...) {
            plan.stage_valid = false;   // (rings may hold part of the window)
            ring_table.valid = false;
            counters_dirty = true;
            throw;
        }
    }

    // Rings of at least `cap` floats each for the plan in hand (execute(), begin_program_stream); what they held does not
    // survive a re-allocation.
    void grow_rings(uint64_t cap) {
        cap = std::max(cap, ring_cap);
        const size_t bytes = (size_t)plan.sp.n_rings * cap * sizeof(float);
        if (cap <= ring_cap && bytes <= d_rings.bytes) return;
        d_rings.ensure(bytes);
        ring_cap = cap;
        plan.stage_valid = false;
        ring_table.valid = false;
    }

    // The one step that changes state before the call's windows are decided: the rings get the size the call needs and are
    // kept (FR_RING_KEEP: what the repair must rebuild is returned) or grown.  Fills in what callplan.hpp asks about them.
    RingRepair prepare_rings(Call &c, uint64_t ring_frames = 0) {
        const StagedPlan &sp = plan.sp;
        ring_state = RingState{};
        if (ring_keep) ring_state.inert = ring_keep_inert();
        c.keep_on = ring_keep && ring_state.inert.empty();
        RingRepair repair;
        if (sp.feedback && history_frames != 0)
            throw Error(FR_ERR_UNSUPPORTED, "feedback through Delay needs the full input history (fr_config.history_frames = 0)");
        if (!sp.uses_rings()) return repair;
        const uint64_t cap = ring_capacity(sp, std::max(c.n_times, ring_frames));   // (ring_frames: the calls a zero-frame bring-up is for)
        const bool table_was_valid = ring_table.valid;
        ring_table.valid = false;            // (until the call is through: a failure leaves nothing to keep)
        if (c.keep_on) {
            // (FR_RING_KEEP: the rings this plan finds in the table stay, the others are brought up to idx by the repair,
            //  and the call itself always runs in its steady form)
            const bool fits = cap <= ring_cap && (size_t)sp.n_rings * ring_cap * sizeof(float) <= d_rings.bytes;
            if (plan.stage_valid && plan.stage_end == c.idx && fits && table_was_valid && ring_table.end == c.idx &&
                ring_table.rings.size() == sp.n_rings) {
                ring_state.kept = sp.n_rings;
                ring_state.repair_from = c.idx;
            } else {
                repair = keep_rings(cap, c.idx, table_was_valid, c.st);
                c.repair_replay = repair.replay;
            }
        } else {
            grow_rings(cap);
            c.rings_valid = plan.stage_valid && plan.stage_end == c.idx;
            if (ring_keep) (c.rings_valid ? ring_state.kept : ring_state.rebuilt) = sp.n_rings;
        }
        return repair;
    }

    // ---- bank launches ----
    // `trk`: where a voice that reads tracks finds them for a window (a span of the track history's ring), instead of the
    // call's own matrix
    struct TrackSrc { const float *p; uint64_t stride; uint32_t limit; };
    // One launch's window and voices.  `tile_off` >= 0: a tile of the exchange window (b0 = x0 + tile_off), written to the
    // tile-major workspace.  `v0`, `nv`: a run of the stage's voices (a repair renders only the voices whose rings it
    // rebuilds; parameters and rows are voice-major, so a run is the same launch at offset pointers).
    struct BankPart {
        uint64_t b0, blen;
        int64_t tile_off;
        const TrackSrc *trk;
        uint32_t v0, nv;
        const BankPlan &bp;
    };

    // The caller's row of input `slot`, deferred to the bank launches (Deferred): a launch over the call's own frames reads
    // it in place -- `len` frames from column `off` -- and the first bank on the slot appends them to the history (a tile of
    // the exchange window: its own part, once per tile).
    void take_deferred_row(uint32_t slot, uint64_t off, uint64_t len, bool tile, BankArgs &a) {
        for (Deferred &d : deferred) {
            if (d.slot != slot) continue;
            a.time = d.src + off;
            a.time_skip = 0;
            a.time_valid = len;
            if (tile) {
                a.hist_dst = (d.dst && d.appended_tile != (int64_t)off) ? d.dst + off : nullptr;
                d.appended_tile = (int64_t)off;
            } else {
                a.hist_dst = d.dst;
                d.dst = nullptr;
            }
        }
    }

    // One bank launch over the window [b0, b0 + blen): the arguments every kernel family shares, then the family's launch.
    void launch_bank_part(const Call &c, BankStage &bs, uint64_t b0, uint64_t blen, int64_t tile_off, const TrackSrc *trk, uint32_t v0 = 0, uint32_t nv = UINT32_MAX) {
        const bool whole = v0 == 0 && nv >= bs.grp.rows.size();
        if (whole) nv = (uint32_t)bs.grp.rows.size();
        else if (bs.grp.general || (uint64_t)v0 + nv > bs.grp.rows.size()) throw Error(FR_ERR_DEVICE, "internal: a run of voices the bank stage cannot launch");
        const BankPlan bp = plan_bank_launch(bs, blen, flag_out.host_flags != nullptr, nv);   // (the one rule, asked about the run's voices)
        const BankPart part{b0, blen, tile_off, trk, v0, nv, bp};
        BankArgs a{};
        a.params = bs.d_params.as<float2>() + ((size_t)v0 << bs.grp.log2_p);
        input_window(bs.grp.input_slot, b0, blen, a.time, a.time_skip, a.time_valid);   // time-slot history for the window
        if (tile_off < 0 && b0 == c.idx && blen == c.n_times) take_deferred_row(bs.grp.input_slot, 0, c.n_times, false, a);   // (direct output, or a ring in steady state)
        if (tile_off >= 0 && c.x_window_is_call()) take_deferred_row(bs.grp.input_slot, (uint64_t)tile_off, blen, true, a);   // a tile of the call itself
        a.rows = bs.d_rows.as<uint32_t>() + v0;
        if (bs.grp.to_ring) {
            a.out = d_rings.as<float>();
            a.out_stride = ring_cap;
            a.ring_mask = ring_cap - 1;
            a.ring_t0 = b0;
        } else if (bs.grp.to_ws) {
            a.out = d_ws.as<float>() + plan.sp.split.size() * (uint64_t)(tile_off > 0 ? tile_off : 0);   // tile-major workspace
            a.out_stride = blen;
        } else {
            a.out = c.dst;
            a.out_stride = c.n_times;
        }
        a.n_voices = nv;
        a.log2_p = bs.grp.log2_p;
        a.n_times = blen;
        a.fast_ok = bs.grp.fast_ok ? 1u : 0u;
        a.voices_per_wave = part.bp.voices_per_wave;
        if (bs.grp.jit) launch_compiled_bank(c, bs, part, a);
        else if (bs.grp.general) launch_general_bank(c, bs, part, a);
        else launch_template_bank(c, bs, part, a);
    }

    // Compiled voices (jit_bank): every input row over the same window; few voices on a short call as pieces, added up in
    // the tree's order by the combine pass.
    void launch_compiled_bank(const Call &c, BankStage &bs, const BankPart &pt, const BankArgs &a) {
        const BankPlan &bp = pt.bp;
        JitBankArgs j{};
        j.params = bs.d_params.as<float>() + ((size_t)pt.v0 << bs.grp.log2_p) * bs.grp.k;
        for (size_t i = 0; i < bs.grp.shape.input_slots.size(); ++i)
            input_window(bs.grp.shape.input_slots[i], pt.b0, pt.blen, j.in[i], j.in_skip[i], j.in_valid[i]);
        j.out = a.out;
        j.rows = a.rows;
        j.out_stride = a.out_stride;
        j.ring_mask = a.ring_mask;
        j.ring_t0 = a.ring_t0;
        j.n_times = pt.blen;
        j.n_voices = a.n_voices << bp.pieces_log2;
        j.log2_p = bp.chunk_log2;
        j.tiles = (uint32_t)((pt.blen + 63) / 64);
        j.nblocks = (uint32_t)bp.jit_blocks;
        j.voices_per_wave = bp.voices_per_wave;
        j.fract_ok = a.fast_ok;
        if (bp.pieces_log2) {   // every voice as pieces, to the kernel rows of a workspace, added up below in the tree's order
            used_scratch = true;   // (the pieces' workspace is shared between calls: no overlap with the next one on another stream)
            d_chunk_ws.ensure(bp.ws_floats * sizeof(float));
            if (d_chunk_rows_n < j.n_voices) {
                std::vector<uint32_t> seq(std::max<uint32_t>(j.n_voices, 4096));
                for (uint32_t i = 0; i < seq.size(); ++i) seq[i] = i;
                d_chunk_rows.ensure(seq.size() * sizeof(uint32_t));
                HIP_CHECK(hipMemcpyAsync(d_chunk_rows.p, seq.data(), seq.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c.st));
                HIP_CHECK(hipStreamSynchronize(c.st));   // (`seq` is a stack object; once per growth)
                d_chunk_rows_n = (uint32_t)seq.size();
            }
            j.out = d_chunk_ws.as<float>();
            j.rows = d_chunk_rows.as<uint32_t>();
            j.out_stride = pt.blen;
        }
        if (bs.grp.tracks && pt.trk) {
            j.tracks = pt.trk->p;
            j.track_stride = pt.trk->stride;
            j.track_limit = pt.trk->limit;
        } else if (bs.grp.tracks && call_tracks) {
            if (pt.b0 != c.idx || pt.blen != c.n_times) throw Error(FR_ERR_UNSUPPORTED, "internal: a voice that reads tracks rendered over another window than the call's");
            j.tracks = call_tracks;
            j.track_stride = call_track_stride;
            j.track_limit = (uint32_t)std::min<uint64_t>((uint64_t)track_from + call_track_rows, 0xFFFFFFFFull);
        }
        note_bank_launch(bp, bs, pt.nv, pt.blen, flag_out.host_flags != nullptr);
        Scope sc(this, &t_bank, c.st);
        HIP_CHECK(launch_jit_bank(*bs.jit, j, c.st));
        if (bp.pieces_log2) {
            ChunkCombineArgs cc{};
            cc.ws = d_chunk_ws.as<float>();
            cc.out = a.out;
            cc.rows = a.rows;
            cc.out_stride = a.out_stride;
            cc.n_times = pt.blen;
            cc.n_voices = a.n_voices;
            cc.log2_c = bp.pieces_log2;
            HIP_CHECK(launch_chunk_combine(cc, c.st));
        }
        sc.done();
    }

    // General trees (gbank): the schedule kernel.
    void launch_general_bank(const Call &c, BankStage &bs, const BankPart &pt, BankArgs &a) {
        a.groups = bs.d_groups.as<uint32_t>();
        a.group_off = bs.d_group_off.as<uint32_t>();
        a.hist_dst = nullptr;   // (the schedule kernel does not append history)
        note_bank_launch(pt.bp, bs, pt.nv, pt.blen, flag_out.host_flags != nullptr);
        Scope sc(this, &t_bank, c.st);
        HIP_CHECK(launch_gbank(a, c.st));
        sc.done();
    }

    // Balanced template voices: the hand-written kernels, in the shape bankplan.hpp picked.
    void launch_template_bank(const Call &c, BankStage &bs, const BankPart &pt, BankArgs &a) {
        const BankPlan &bp = pt.bp;
        if (a.hist_dst && !bp.appends_rows) throw Error(FR_ERR_DEVICE, "internal: deferred history append on a short call");
        a.chunk_log2 = bp.chunk_log2;
        a.frames_per_lane = bp.frames_per_lane;
        a.waves_per_group = bp.waves_per_group;
        a.small_call = bp.small_call;
        a.leaf_variant = bank_tune.leaf_variant;
        if (flag_out.host_flags) {
            if (!bp.publishes_rows) throw Error(FR_ERR_DEVICE, "internal: a bank launch cannot publish row flags");
            a.host_flags = flag_out.host_flags;
            a.row_done = flag_out.row_done;
            a.flag_value = flag_out.value;
        }
        if (bp.ws_floats) {
            used_scratch = true;
            d_bank_ws.ensure(bp.ws_floats * sizeof(float));
            a.ws = d_bank_ws.as<float>();
            if (bp.ticket_words) a.tickets = ticket_counters(bp.ticket_words, c.st);
        }
        note_bank_launch(bp, bs, pt.nv, pt.blen, flag_out.host_flags != nullptr);
        Scope sc(this, &t_bank, c.st);
        HIP_CHECK(launch_bank(a, c.st));
        sc.done();
    }

    // A voice that reads tracks over a window that starts before idx (it feeds a delay line: the call after a seek, an edit
    // or a ring growth) is launched per span: the frames before idx from the track history, cut again where its ring
    // wraps, then the call's own frames as in steady state.  Every span is the same generated kernel.
    void launch_bank_window(const Call &c, BankStage &bs, uint64_t b0, uint64_t blen, int64_t tile_off) {
        if (!(bs.grp.tracks && tail_on() && tile_off < 0 && b0 < c.idx && b0 + blen == c.idx + c.n_times)) {
            launch_bank_part(c, bs, b0, blen, tile_off, nullptr);
            return;
        }
        for (uint64_t s0 = b0; s0 < c.idx;) {
            const uint64_t pos = s0 & (tail_cap - 1);
            const uint64_t len = std::min(c.idx - s0, tail_cap - pos);
            TrackSrc ts{nullptr, tail_cap, 0};
            if (tail_rows) {
                ts.p = reinterpret_cast<const float *>(reinterpret_cast<uintptr_t>(d_tail.as<float>() + pos) - (uintptr_t)track_from * tail_cap * sizeof(float));
                ts.limit = (uint32_t)std::min<uint64_t>((uint64_t)track_from + tail_rows, 0xFFFFFFFFull);
            }
            launch_bank_part(c, bs, s0, len, -1, &ts);
            s0 += len;
        }
        launch_bank_part(c, bs, c.idx, c.n_times, -1, nullptr);
    }

    // ---- stage launches ----
    // The input table of the call's stage launches (the inputs as they stand when the launches are enqueued).
    std::vector<DevInput> stage_tab;
    void fill_stage_tab(hipStream_t st) {
        const StagedPlan &sp = plan.sp;
        stage_tab.resize(sp.input_slots.size());
        for (size_t i = 0; i < stage_tab.size(); ++i) stage_tab[i] = dev_input(sp.input_slots[i]);
        if (stage_tab.size() > STAGE_INLINE_INPUTS) {   // rare: more input slots than fit in the kernel arguments
            d_in_table_stage.ensure(stage_tab.size() * sizeof(DevInput));
            HIP_CHECK(hipMemcpyAsync(d_in_table_stage.p, stage_tab.data(), stage_tab.size() * sizeof(DevInput), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));   // (the table is rewritten by the next fill)
        }
    }
    // What a stage launch is for (StageLaunchNote::form) and the frames its threads stride by (0: one frame per thread).
    // `sweep` (FR_LOOP_DYN): the frames per sweep of a stage_sweep_kernel launch (0: stage_kernel / jit_stage); `window`: the
    // launch is one window of the windows form.
    struct StageLaunch { const char *form; uint64_t stride; uint32_t sweep = 0; bool window = false; };
    // The fields JitStageArgs and StageArgs share.
    template <class Args>
    void fill_stage_args(Args &a, const Call &c, const StageLaunch &how, uint64_t s0, uint64_t slen, bool carry_only) const {
        a.rings = d_rings.as<float>();
        a.ring_mask = ring_cap ? ring_cap - 1 : 0;
        a.n_inputs = (uint32_t)stage_tab.size();
        a.out = c.dst;
        a.n_times = c.n_times;
        a.idx = c.idx;
        a.w0 = s0;
        a.w_len = slen;
        a.stride = how.stride;
        a.carry_only = carry_only ? 1u : 0u;
    }
    // Programs [first, first + count) over the frames [s0, s0 + slen), in launches of at most 65535 programs (grid.y).
    void launch_range(const Call &c, const StageLaunch &how, uint32_t first, uint32_t count, uint64_t s0, uint64_t slen) {
        const StagedPlan &sp = plan.sp;
        const bool carry = how.stride && sp.feedback, carry_only = carry && sp.fused_carry_only;
        // (loop tiles: the rule looked at the fused programs, which are all a feedback plan ever launches strided)
        const uint32_t tile = carry_only && how.stride == sp.fused_stride && first >= sp.fused_first && first + count <= sp.fused_first + sp.fused_count
                                  ? plan.loop_tile.frames : 0u;
        const size_t n_inline = std::min<size_t>(stage_tab.size(), STAGE_INLINE_INPUTS);
        if (count && stage_launches.size() < 256)
            stage_launches.push_back({how.form, plan.stage_jit != nullptr, count, slen, how.sweep ? how.sweep : how.stride, carry, carry_only,
                                      stage_tab.size() > STAGE_INLINE_INPUTS, (count - 1) / 65535u + 1, tile != 0, how.sweep ? 1u : how.window ? 2u : 0u});
        for (uint32_t off = 0; off < count; off += 65535u) {
            const uint32_t n = std::min<uint32_t>(count - off, 65535u);
            Scope sc(this, &t_stage, c.st);
            if (plan.stage_jit) {
                JitStageArgs a{};
                fill_stage_args(a, c, how, s0, slen, carry_only);
                a.ptab = plan.d_ptab.as<uint32_t>();
                a.progs = plan.d_jprogs.as<JitStageProg>() + first + off;
                a.inputs = reinterpret_cast<const JitInput *>(d_in_table_stage.as<DevInput>());
                for (size_t i = 0; i < n_inline; ++i) a.inline_inputs[i] = JitInput{stage_tab[i].data, stage_tab[i].base, stage_tab[i].len};
                a.tile = tile;
                HIP_CHECK(launch_jit_stage(*plan.stage_jit, a, n, c.st));
            } else {
                StageArgs a{};
                fill_stage_args(a, c, how, s0, slen, carry_only);
                a.instrs = plan.d_instrs.as<StageInstr>();
                a.progs = plan.d_progs.as<StageProg>() + first + off;
                a.n_progs = n;
                a.inputs = d_in_table_stage.as<DevInput>();
                for (size_t i = 0; i < n_inline; ++i) a.inline_inputs[i] = stage_tab[i];
                a.use_carry = carry ? 1u : 0u;
                a.sparkle = mirror.sparkle ? 1u : 0u;
                a.tile = tile;
                a.sweep = how.sweep;
                HIP_CHECK(how.sweep ? launch_stage_sweep(a, c.st) : launch_stage(a, c.st));
            }
            sc.done();
        }
    }
    // A feedback plan's fused form: a strided launch per level.
    void launch_fused_levels(const Call &c, const char *form, uint64_t s0, uint64_t slen) {
        const StagedPlan &sp = plan.sp;
        // A sweep plan (FR_LOOP_DYN, callplan.hpp loop_sweep): a sweep launch per level, or the windows form -- the window cut into
        // W frames, the levels inside each.  The strided form is not valid for it (there is no stride).
        const LoopSweep &ls = plan.loop_sweep;
        if (sp.fused_sweep && ls.form == LoopSweep::none) throw Error(FR_ERR_DEVICE, "internal: a sweep plan without a launch form");
        if (ls.form == LoopSweep::windows) {
            for (uint64_t done = 0; done < slen;) {
                const uint64_t len = std::min<uint64_t>(ls.sweep, slen - done);
                for (size_t l = 0; l + 1 < sp.fused_level_first.size(); ++l)
                    launch_range(c, {form, 0, 0, true}, sp.fused_first + sp.fused_level_first[l], sp.fused_level_first[l + 1] - sp.fused_level_first[l], s0 + done, len);
                done += len;
            }
            return;
        }
        const uint32_t sweep = ls.form == LoopSweep::kernel ? ls.frames : 0u;
        for (size_t l = 0; l + 1 < sp.fused_level_first.size(); ++l)
            launch_range(c, {form, sp.fused_stride, sweep}, sp.fused_first + sp.fused_level_first[l], sp.fused_level_first[l + 1] - sp.fused_level_first[l], s0, slen);
    }

    // ---- the call's phases ----
    // Kept rings (FR_RING_KEEP): the rings to rebuild are brought up to idx -- their voices, then their programs level by
    // level, nothing written to the output -- over the look-back window, or for a feedback plan's loops from frame 0
    void repair_rings(const Call &c, const RingRepair &repair) {
        if (repair.empty()) return;
        fill_stage_tab(c.st);
        bank_form = repair.replay ? "replay" : "repair";
        const StageLaunch how{bank_form, repair.replay ? plan.sp.fused_stride : 0};
        for (uint64_t c0 = repair.from; c0 < c.idx;) {
            const uint64_t len = repair.replay ? std::min<uint64_t>(FB_CHUNK, c.idx - c0) : c.idx - c0;
            for (const RingRepair::Run &run : repair.voices) launch_bank_part(c, plan.banks[run.stage], c0, len, -1, nullptr, run.first, run.count);
            for (const auto &level : repair.levels)
                for (const auto &run : level) launch_range(c, how, run.first, run.second, c0, len);
            c0 += len;
        }
        bank_form = "call";   // (a failure in between: execute() starts every call with it)
    }
    // A feedback plan whose rings are not current: every frame from 0 replayed in chunks -- the ring-bound banks and the fused
    // programs over [c0, c0 + len), nothing written to the output -- before the call's own frames run in steady-state form.
    void replay_feedback(const Call &c) {
        if (!c.w.fb_replay) return;
        fill_stage_tab(c.st);
        for (uint64_t c0 = 0; c0 < c.idx; c0 += FB_CHUNK) {
            const uint64_t len = std::min<uint64_t>(FB_CHUNK, c.idx - c0);
            for (BankStage &bs : plan.banks)
                if (bs.grp.to_ring) launch_bank_window(c, bs, c0, len, -1);
            launch_fused_levels(c, "replay", c0, len);
        }
    }
    // Split voices (partial-block sharding).  The exchange window first, tile by tile, every tile's bank kernels on the call's
    // stream; then the tiles' exchanges on the exchange stream, each behind its tile's event: tile i's exchange runs under the
    // bank kernels of tiles i + 1 ... (also with a transport that blocks the host: the kernels are all enqueued before the
    // first exchange starts).  One tile = the serial form of round 2, all on the call's stream.
    void exchange_split_voices(const Call &c) {
        const StagedPlan &sp = plan.sp;
        if (sp.split.empty()) return;
        used_scratch = true;
        d_ws.ensure(sp.split.size() * c.w.xlen * sizeof(float));
        d_xrecv.ensure(sp.split.size() * c.w.xlen * sizeof(float));
        if (c.pipelined()) {
            if (!xstream) HIP_CHECK(hipStreamCreateWithFlags(&xstream, hipStreamNonBlocking));
            while (x_events.size() < c.xt.count + 1) {
                hipEvent_t e;
                HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                x_events.push_back(e);
            }
        }
        ++exchange_calls;
        exchange_tiles += c.xt.count;
        for (uint32_t ti = 0; ti < c.xt.count; ++ti) {
            for (BankStage &bs : plan.banks)
                if (bs.grp.to_ws) launch_bank_window(c, bs, c.w.x0 + c.xt.offset(ti), c.xt.frames(ti), (int64_t)c.xt.offset(ti));
            if (c.pipelined()) HIP_CHECK(hipEventRecord(x_events[ti], c.st));
        }
        for (uint32_t ti = 0; ti < c.xt.count; ++ti) {
            if (c.pipelined()) HIP_CHECK(hipStreamWaitEvent(xstream, x_events[ti], 0));
            run_exchange(c.dst, c.n_times, c.idx, c.w.x0, c.xt.offset(ti), c.xt.frames(ti), c.pipelined() ? xstream : c.st);
        }
        for (Deferred &d : deferred)
            if (d.appended_tile >= 0) d.dst = nullptr;   // appended tile by tile
    }
    // Everything else (voices that stay whole on this rank, unsharded plans) -- overlapping the exchange's tail; the call's
    // stream then goes on only behind the last tile's exchange.
    void launch_whole_banks(const Call &c) {
        for (BankStage &bs : plan.banks) {
            if (bs.grp.to_ws) continue;
            const bool ring = bs.grp.to_ring;
            launch_bank_window(c, bs, ring ? c.w.w0 : c.idx, ring ? c.w.w_len : c.n_times, -1);
        }
        if (c.pipelined()) {
            HIP_CHECK(hipEventRecord(x_events[c.xt.count], xstream));
            HIP_CHECK(hipStreamWaitEvent(c.st, x_events[c.xt.count], 0));
        }
        for (const Deferred &d : deferred)
            if (d.dst) throw Error(FR_ERR_DEVICE, "internal: an input row deferred to the bank launch was not appended");
    }
    // The call's stage programs, in the form callplan.hpp picked (StageForm).
    void launch_stage_programs(const Call &c) {
        const StagedPlan &sp = plan.sp;
        if (c.form.kind == StageForm::none) return;
        fill_stage_tab(c.st);
        switch (c.form.kind) {
        case StageForm::feedback:
            launch_fused_levels(c, "feedback", c.idx, c.n_times);
            launch_range(c, {"copy", 0}, sp.post_first, sp.post_count, c.idx, c.n_times);
            break;
        case StageForm::strided:
            launch_range(c, {"strided", sp.fused_stride}, sp.fused_first, sp.fused_count, c.idx, c.n_times);
            break;
        case StageForm::fused:
            for (uint64_t done = 0; done < c.n_times;) {   // by frames still to do: no sum that could wrap
                const uint64_t len = std::min<uint64_t>(c.form.fused_step, c.n_times - done);
                launch_range(c, {"fused", 0}, sp.fused_first, sp.fused_count, c.idx + done, len);
                done += len;
            }
            break;
        default:
            for (size_t l = 0; l + 1 < sp.level_first.size(); ++l)
                launch_range(c, {"levels", 0}, sp.level_first[l], sp.level_first[l + 1] - sp.level_first[l], c.w.w0, c.w.w_len);
        }
    }
    // The rings now hold the plan's frames up to the call's end.
    void commit_rings(const Call &c) {
        if (!plan.sp.uses_rings()) return;
        plan.stage_valid = true;
        plan.stage_end = c.idx + c.n_times;
        if (c.keep_on) {                   // the call's frames are in; the oldest ones of a full ring are gone
            ring_table.end = c.idx + c.n_times;
            const uint64_t oldest = ring_table.end > ring_cap ? ring_table.end - ring_cap : 0;
            for (RingEntry &e : ring_table.rings) e.valid_from = std::max(e.valid_from, oldest);
            ring_table.valid = true;
        }
    }

    void run_pull(float *d_dst, uint32_t n_slots, uint64_t n_times, uint64_t idx, hipStream_t st) {
        // input table for this call
        std::vector<DevInput> tab(plan.input_slots.size());
        for (size_t i = 0; i < tab.size(); ++i) tab[i] = dev_input(plan.input_slots[i]);
        d_in_table.ensure(std::max<size_t>(tab.size(), 1) * sizeof(DevInput));
        if (!tab.empty()) {
            HIP_CHECK(hipMemcpyAsync(d_in_table.p, tab.data(), tab.size() * sizeof(DevInput), hipMemcpyHostToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
        const uint64_t depth = std::max<uint32_t>(plan.max_depth, 1);
        // pull rows are processed as contiguous runs of rows; stack workspace bounded to ~1 GiB
        const uint64_t budget = 1ull << 30;
        uint64_t chunk = std::max<uint64_t>(budget / (depth * 16), 256);
        size_t i = 0;
        while (i < plan.pull_rows.size()) {
            size_t j = i + 1;
            while (j < plan.pull_rows.size() && plan.pull_rows[j] == plan.pull_rows[j - 1] + 1) ++j;
            uint64_t first = (uint64_t)plan.pull_rows[i] * n_times;
            uint64_t total = (uint64_t)(j - i) * n_times;
            for (uint64_t off = 0; off < total; off += chunk) {
                uint64_t cnt = std::min(chunk, total - off);
                d_stack_node.ensure(depth * cnt * sizeof(uint32_t));
                d_stack_time.ensure(depth * cnt * sizeof(uint64_t));
                d_stack_val.ensure(depth * cnt * sizeof(float));
                PullArgs a{};
                a.nodes = plan.d_nodes.as<DevNode>();
                a.outputs = plan.d_roots.as<uint32_t>();
                a.inputs = d_in_table.as<DevInput>();
                a.n_inputs = (uint32_t)tab.size();
                a.out = d_dst;
                a.n_slots = n_slots;
                a.n_times = n_times;
                a.idx = idx;
                a.first = first + off;
                a.count = cnt;
                a.sparkle = mirror.sparkle ? 1u : 0u;
                a.st_node = d_stack_node.as<uint32_t>();
                a.st_time = d_stack_time.as<uint64_t>();
                a.st_val = d_stack_val.as<float>();
                Scope sc(this, &t_pull, st);
                HIP_CHECK(launch_pull(a, st));
                sc.done();
            }
            i = j;
        }
    }
};

// fr_stream_begin of a plan with programs (FR_STREAM_PROGRAMS): the rule, the per-voice program tables, the rings' size.  The
// resident launch starts with the first block (seek_program_stream).
void fr_renderer::begin_program_stream(uint32_t n_slots) {
    const StagedPlan &sp = plan.sp;
    if (!plan_current(n_slots)) throw Error(FR_ERR_UNSUPPORTED, "block streaming: the plan is not current");
    StreamPlan s = plan_stream_now();
    if (!s.servable) throw Error(FR_ERR_UNSUPPORTED, "block streaming (FR_STREAM_PROGRAMS): " + s.reason);
    // a stream that stores its rows (FR_STREAM_STORE): the slots it streams as the store stands (streamstore.hpp); a block may add more
    std::vector<uint32_t> row_slots = s.input_slots;
    if (s.store) {
        std::string why;
        if (!stream_store_slots(s.input_slots, slots, 0, row_slots, &why)) throw Error(FR_ERR_UNSUPPORTED, "block streaming (FR_STREAM_STORE): " + why);
    }
    if (s.banks.size() != plan.banks.size() || s.banks.size() > BANK_STREAM_BANKS) throw Error(FR_ERR_DEVICE, "internal: the stream's banks are not the plan's");
    // a plan without a voice (FR_STREAM_EFFECTS): its segments are the launch's workgroups, one wave each; no parameters, workspace or tickets
    if ((s.voices == 0) != (s.segments != 0) || (s.segments && (!plan.banks.empty() || s.voice_first.size() != (size_t)s.segments + 2 || s.segments > BANK_STREAM_WGS)))
        throw Error(FR_ERR_DEVICE, "internal: a stream with neither voices nor segments");
    for (size_t i = 0; i < plan.banks.size(); ++i) {
        const BankLaunch &grp = plan.banks[i].grp;
        if (grp.rows.size() != s.banks[i].voices) throw Error(FR_ERR_DEVICE, "internal: the stream's banks are not the plan's");
        for (uint32_t row : grp.rows)
            if (row >= (grp.to_ring ? sp.n_rings : n_slots)) throw Error(FR_ERR_DEVICE, "internal: a streamed voice's row out of bounds");
    }
    Stream::Open o;
    o.launch = stream_launch(sp, s);
    o.store = s.store;
    if (o.store) o.launch.n_rows = (uint32_t)row_slots.size();
    upload_stream_programs(s, o.launch, row_slots, n_slots);
    begin_program_stream_rest(std::move(o), std::move(s), n_slots);
}

// The stream's own copy of the plan's programs for a launch whose streamed rows are the slots `row_slots`, in that order
// (StreamPlan::input_slots; a stream that stores its rows: streamstore.hpp stream_store_slots, again whenever the set grows).
void fr_renderer::upload_stream_programs(const StreamPlan &s, const StreamLaunch &l, const std::vector<uint32_t> &row_slots, uint32_t n_slots) {
    const StagedPlan &sp = plan.sp;
    std::vector<StageProg> progs(s.progs.size());
    for (size_t i = 0; i < progs.size(); ++i) {
        progs[i] = sp.progs[s.progs[i]];
        const StageProg &pg = progs[i];
        if ((uint64_t)pg.first_instr + pg.n_instr > sp.instrs.size() || (pg.dst_ring != 0xFFFFFFFFu && pg.dst_ring >= sp.n_rings) || pg.out_row >= (int64_t)n_slots)
            throw Error(FR_ERR_DEVICE, "internal: a streamed program out of the plan's bounds");
        for (uint32_t k = 0; k < pg.n_instr; ++k) {
            const StageInstr &in = sp.instrs[pg.first_instr + k];
            if ((in.op == S_READ || in.op == S_READ_DYN || in.op == S_STORE) && in.buf >= sp.n_rings) throw Error(FR_ERR_DEVICE, "internal: a streamed program reads a ring the plan does not have");
        }
    }
    // the stream's own copy of the programs' instructions (StreamLaunch::own_instrs): the operand of S_INPUT -- and of S_READ_INPUT
    // and S_READ_INPUT_DYN, FR_STREAM_HISTORY -- the streamed row (the position of its slot in row_slots) instead of the plan's
    // input index; a loop program's store slots; in a plan with a sweep walk (FR_STREAM_SWEEP) S_READ_DYN's imm, a sweep plan's proven
    // bound, becomes the store slot + 1 of an own ring (stream_sweep_prepare) and 0 everywhere else -- the kernel reads it as that.
    // (The plan's own instructions, which the ordinary path runs, are not touched.)
    std::vector<StageInstr> instrs;
    if (l.own_instrs) {
        if (row_slots.size() > BANK_STREAM_ROWS) throw Error(FR_ERR_DEVICE, "internal: more streamed rows than the kernel takes");
        for (size_t i = 0; i < progs.size(); ++i) {
            StageProg &pg = progs[i];
            std::vector<StageInstr> own;
            for (uint32_t k = 0; k < pg.n_instr; ++k) {
                StageInstr in = sp.instrs[pg.first_instr + k];
                if (in.op == S_INPUT || in.op == S_READ_INPUT || in.op == S_READ_INPUT_DYN) {
                    const auto it = in.imm < sp.input_slots.size() ? std::find(row_slots.begin(), row_slots.end(), sp.input_slots[in.imm]) : row_slots.end();
                    if (it == row_slots.end()) throw Error(FR_ERR_DEVICE, "internal: a streamed program reads a slot the stream does not feed");
                    in.imm = (uint32_t)(it - row_slots.begin());
                }
                if (in.op == S_READ_DYN && s.has_sweep() && s.sweep_width[i] == 0) in.imm = 0;
                own.push_back(in);
            }
            if (s.sweep_width[i] != 0 && (s.sweep_width[i] != s.loop_stride[i] || !stream_sweep_prepare(pg, own) || pg.pad[0] != s.sweep_width[i]))
                throw Error(FR_ERR_DEVICE, "internal: a sweep program the stream cannot prepare");
            if (s.sweep_width[i] == 0 && s.loop_stride[i] != 0 && (!stream_loop_prepare(pg, own) || pg.pad[0] != s.loop_stride[i]))
                throw Error(FR_ERR_DEVICE, "internal: a loop program the stream cannot prepare");
            pg.first_instr = (uint32_t)instrs.size();
            instrs.insert(instrs.end(), own.begin(), own.end());
        }
        strm.d_instrs.ensure(std::max<size_t>(instrs.size(), 1) * sizeof(StageInstr));
        if (!instrs.empty()) HIP_CHECK(hipMemcpyAsync(strm.d_instrs.p, instrs.data(), instrs.size() * sizeof(StageInstr), hipMemcpyHostToDevice, stream));
    }
    // the leaf banks' programs (FR_STREAM_LEAVES), bank after bank: LEAF_IN's operand the streamed row, as S_INPUT's
    std::vector<LeafInstr> leaf_ins;
    for (const LeafProgram &lp : s.leaf_progs)
        for (LeafInstr in : lp.ins) {
            for (int side = 0; side < 2; ++side) {
                if ((side ? in.kb : in.ka) != LEAF_IN) continue;
                uint32_t &v = side ? in.b : in.a;
                const auto it = v < lp.input_slots.size() ? std::find(row_slots.begin(), row_slots.end(), lp.input_slots[v]) : row_slots.end();
                if (it == row_slots.end() || row_slots.size() > BANK_STREAM_ROWS) throw Error(FR_ERR_DEVICE, "internal: a streamed leaf reads a slot the stream does not feed");
                v = (uint32_t)(it - row_slots.begin());
            }
            for (int side = 0; side < 2; ++side) {               // a track operand: its place in the bank's track columns (kernels.hpp StreamTrackArgs::Bank::cols)
                uint8_t &kind = side ? in.kb : in.ka;
                if (kind != LEAF_TRK && kind != LEAF_TRK_LIT) continue;
                uint32_t &v = side ? in.b : in.a;
                const uint32_t q = lp.track_index(kind, v);
                if (q >= lp.track_cols.size() || q >= BANK_STREAM_LEAF_TRACKS) throw Error(FR_ERR_DEVICE, "internal: a streamed leaf reads a track the program does not list");
                kind = LEAF_TRK;
                v = q;
            }
            if (in.dst >= BANK_STREAM_LEAF_REGS || (in.ka == LEAF_REG && in.a >= BANK_STREAM_LEAF_REGS) || (in.kb == LEAF_REG && in.b >= BANK_STREAM_LEAF_REGS) ||
                (in.ka == LEAF_PARAM && in.a >= lp.k) || (in.kb == LEAF_PARAM && in.b >= lp.k))
                throw Error(FR_ERR_DEVICE, "internal: a leaf program out of the interpreter's bounds");
            leaf_ins.push_back(in);
        }
    if (!leaf_ins.empty()) {
        strm.d_leaf.ensure(leaf_ins.size() * sizeof(LeafInstr));
        HIP_CHECK(hipMemcpyAsync(strm.d_leaf.p, leaf_ins.data(), leaf_ins.size() * sizeof(LeafInstr), hipMemcpyHostToDevice, stream));
    }
    strm.d_progs.ensure(std::max<size_t>(progs.size(), 1) * sizeof(StageProg));
    strm.d_vfirst.ensure(s.voice_first.size() * sizeof(uint32_t));
    if (!progs.empty()) HIP_CHECK(hipMemcpyAsync(strm.d_progs.p, progs.data(), progs.size() * sizeof(StageProg), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(strm.d_vfirst.p, s.voice_first.data(), s.voice_first.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));   // (host vectors go out of scope)
}

// (the rest of fr_stream_begin of a plan with programs: the schedules, the rings' size, the history, the buffers)
void fr_renderer::begin_program_stream_rest(Stream::Open &&o, StreamPlan &&s, uint32_t n_slots) {
    const StagedPlan &sp = plan.sp;
    const StreamLaunch &l = o.launch;
    // schedule banks (FR_STREAM_GENERAL): every voice's schedule stays inside the bank's items and parameters (the rule has
    // validated its stack); the one-item schedules of balanced 32- and 64-partial banks are built and uploaded here, once
    o.sched_at.assign(plan.banks.size(), {SIZE_MAX, SIZE_MAX});
    if (l.schedule_table) {
        std::vector<uint32_t> words;
        for (size_t i = 0; i < plan.banks.size(); ++i) {
            if (!s.banks[i].general) continue;
            const BankLaunch &grp = plan.banks[i].grp;
            std::vector<uint32_t> own_groups, own_off;
            if (!grp.general) stream_balanced_schedule(s.banks[i].voices, grp.log2_p, own_groups, own_off);
            const std::vector<uint32_t> &groups = grp.general ? grp.groups : own_groups, &group_off = grp.general ? grp.group_off : own_off;
            for (uint32_t v = 0; v < s.banks[i].voices; ++v)
                if (!stream_schedule_ok(groups, group_off, v) ||
                    (uint64_t)group_off[2 * v + 1] * 8u + stream_schedule_pairs(groups, group_off, v) > grp.params.size() / 2)
                    throw Error(FR_ERR_DEVICE, "internal: a streamed voice's schedule out of the bank's bounds");
            if (grp.general) {
                if (plan.banks[i].d_groups.bytes < groups.size() * sizeof(uint32_t) || plan.banks[i].d_group_off.bytes < group_off.size() * sizeof(uint32_t))
                    throw Error(FR_ERR_DEVICE, "internal: a general bank without its device schedule");
                continue;
            }
            o.sched_at[i] = {words.size(), words.size() + own_groups.size()};
            words.insert(words.end(), own_groups.begin(), own_groups.end());
            words.insert(words.end(), own_off.begin(), own_off.end());
        }
        strm.d_sched.ensure(std::max<size_t>(words.size(), 1) * sizeof(uint32_t));
        if (!words.empty()) {
            HIP_CHECK(hipMemcpyAsync(strm.d_sched.p, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            HIP_CHECK(hipStreamSynchronize(stream));   // (`words` goes out of scope)
        }
    }
    // rings: the deepest look-back and a block, as execute() sizes them for a 64-frame call (which the seek then finds in place)
    // (a stream that stores its rows sizes them with its first block's bring-up, which keeps what FR_RING_KEEP can keep)
    if (sp.uses_rings() && !o.store) grow_rings(ring_capacity(sp, STREAM_BLOCK));
    // the history of the streamed rows (FR_STREAM_HISTORY): hist_cap frames for each of the n_rows rows, zeroed by every seek.  It
    // needs no books of its own next to streamrows.hpp's: what accept() puts into a block's doorbell for a slot -- the row, its
    // padding, +0.0 for a slot without a row or beyond the vector count -- is, frame for frame, what fr_fill_buffer's input store
    // would answer for that frame ever after (a slot that lags can only be fed again after a seek), and workgroup 0 stores exactly
    // those words.  After a seek the store answers 0.0 for every earlier frame: the zeroed history, and the kernel's frame >= d.
    if (l.hist_cap) {
        if (l.hist_cap < s.input_lookback + STREAM_BLOCK || (l.hist_cap & (l.hist_cap - 1)) != 0) throw Error(FR_ERR_DEVICE, "internal: the input history does not hold the stream's look-back");
        strm.d_hist.ensure((size_t)(o.store ? BANK_STREAM_ROWS : l.n_rows) * l.hist_cap * sizeof(float));   // (store: the set of rows may grow)
    }
    if (s.has_tracks()) strm.h_trk.ensure((size_t)s.track_rows * STREAM_BLOCK * sizeof(float));   // FR_STREAM_TRACKS: a block's track rows
    ensure_stream_buffers(l, n_slots);
    o.prog = true;
    o.plan = std::move(s);
    open_stream(std::move(o), n_slots);
}

// A block that does not continue the previous one (the first block included): the running launch is retired, the rings are
// brought up to idx by the ordinary path -- a call of the frames just before idx after a seek there: every input before idx
// reads 0.0, the look-back window (a feedback plan: the replay from 0) is rebuilt, its output goes nowhere -- and the resident
// launch starts with head = idx.
void fr_renderer::seek_program_stream(uint64_t idx) {
    HIP_CHECK(hipSetDevice(device));
    stop_resident(true);
    const uint32_t n_slots = strm.now.slots;
    const StagedPlan &sp = plan.sp;
    if (!plan_current(n_slots)) throw Error(FR_ERR_DEVICE, "internal: a stream outlived its plan");
    const uint64_t warm = sp.uses_rings() ? std::min<uint64_t>(idx, STREAM_BLOCK) : 0;
    plan.stage_valid = false;                    // whatever the rings hold, they do not hold a seek to idx
    ring_table.valid = false;
    head = UINT64_MAX;
    if (warm) {
        const uint64_t offs[1] = {0};
        const auto snap = snapshot_store(idx - warm);
        try {
            store_inputs(n_slots, warm, idx - warm, nullptr, offs, 0, false, stream);
            d_out.ensure((size_t)n_slots * warm * sizeof(float));
            execute(d_out.as<float>(), n_slots, warm, idx - warm, stream);
        } catch (...) {
            rollback_store(snap);
            throw;
        }
        // the warm-up is no call of the host's: the input vectors it made room for (n_slots * warm, reference.rs:60) are not
        // counted.  (Whatever follows the stream is a seek, which rebuilds the segments from the count.)
        n_vecs = snap.n_vecs;
    }
    plan.stage_valid = false;                    // from here on the rings run ahead of the input store
    ring_table.valid = false;
    start_resident(idx, true);
}

// The resident launch of the open stream of the program path at head = idx, the rings standing at idx.  `empty_history`: every
// frame before idx reads 0.0 (a seek); else the history was filled from the input store (fill_stream_history).
void fr_renderer::start_resident(uint64_t idx, bool empty_history) {
    const uint32_t n_slots = strm.now.slots;
    const StagedPlan &sp = plan.sp;
    const StreamPlan &s = strm.now.plan;
    const StreamLaunch &l = strm.now.launch;
    size_t plan_voices = 0;
    for (const BankStage &b : plan.banks) plan_voices += b.grp.rows.size();
    if ((sp.uses_rings() && (ring_cap < sp.lmax + STREAM_BLOCK || (size_t)sp.n_rings * ring_cap * sizeof(float) > d_rings.bytes)) || s.voices != plan_voices ||
        s.banks.size() != plan.banks.size())
        throw Error(FR_ERR_DEVICE, "internal: the rings do not hold a streamed block's look-back");
    StreamLaunchArgs x{};
    const bool voiceless = s.voices == 0;                        // FR_STREAM_EFFECTS: n_voices = the segments, and `out`; no bank
    x.a = voiceless ? stream_bank_args(nullptr, s.segments, 0, 1) : stream_bank_args(l.bank_table ? nullptr : &plan.banks[0], s.voices, s.chunk_log2, s.chunks);
    StreamProgArgs &p = x.p;
    p.instrs = l.own_instrs ? strm.d_instrs.as<StageInstr>() : plan.d_instrs.as<StageInstr>();
    p.progs = strm.d_progs.as<StageProg>();
    p.voice_first = strm.d_vfirst.as<uint32_t>();
    p.rings = sp.uses_rings() ? d_rings.as<float>() : nullptr;
    p.ring_mask = sp.uses_rings() ? ring_cap - 1 : 0;
    p.n_rings = sp.n_rings;
    p.n_rows = n_slots;
    p.head = idx;
    p.bank_to_ring = !l.bank_table && !voiceless && plan.banks[0].grp.to_ring ? 1u : 0u;   // (a bank table: each bank has its own)
    p.sparkle = mirror.sparkle ? 1u : 0u;
    if (l.hist_cap) {                                            // every frame before idx reads 0.0 after a seek: an empty history, on the launch's stream
        const size_t bytes = (size_t)l.n_rows * l.hist_cap * sizeof(float);
        if (bytes > strm.d_hist.bytes) throw Error(FR_ERR_DEVICE, "internal: the input history does not hold the stream's look-back");
        if (empty_history) HIP_CHECK(hipMemsetAsync(strm.d_hist.p, 0, bytes, stream));
        x.h.hist = strm.d_hist.as<float>();
        x.h.mask = l.hist_cap - 1;
    }
    if (l.bank_table) {
        // the bank table travels in the kernel arguments (and, for schedule banks, a second table of their schedules); chunk
        // sums and tickets are laid out by global voice
        StreamBanksArgs &t = x.t;
        t.n_banks = (uint32_t)s.banks.size();
        for (size_t i = 0; i < s.banks.size(); ++i) {
            const BankStage &b = plan.banks[i];
            const StreamBank &sb = s.banks[i];
            if (b.grp.rows.size() != sb.voices || (!b.grp.general && b.grp.log2_p != sb.log2_p) || (b.grp.general && !sb.general))
                throw Error(FR_ERR_DEVICE, "internal: the stream's banks are not the plan's");
            if (sb.general) {                                    // its schedule: the ordinary launch's device copy, or the stream's own
                const auto &sched_at = strm.now.sched_at;
                x.g.mask |= 1u << i;
                if (b.grp.general) {
                    x.g.bank[i].groups = b.d_groups.as<uint32_t>();
                    x.g.bank[i].group_off = b.d_group_off.as<uint32_t>();
                } else {
                    if (i >= sched_at.size() || sched_at[i].first == SIZE_MAX) throw Error(FR_ERR_DEVICE, "internal: a schedule bank without its schedule");
                    x.g.bank[i].groups = strm.d_sched.as<uint32_t>() + sched_at[i].first;
                    x.g.bank[i].group_off = strm.d_sched.as<uint32_t>() + sched_at[i].second;
                }
            }
            t.bank[i] = {b.d_params.as<float2>(), b.d_rows.as<uint32_t>(), sb.first_wg, sb.first_voice, sb.voices, sb.log2_p, sb.chunk_log2,
                         b.grp.fast_ok ? 1u : 0u, b.grp.to_ring ? 1u : 0u};
        }
        // leaf banks (FR_STREAM_LEAVES): each one's program in d_leaf (upload_stream_programs), its parameter table [voice][P][k] as uploaded
        size_t leaf_at = 0;
        for (size_t i = 0; i < s.leaf_progs.size() && i < s.banks.size(); ++i) {
            const LeafProgram &lp = s.leaf_progs[i];
            if (!s.banks[i].leaf) continue;
            const BankStage &b = plan.banks[i];
            if (!b.grp.jit || (b.grp.tracks && !s.has_tracks()) || lp.k == 0 || lp.k != std::max(b.grp.k, 1u) || lp.ins.size() > BANK_STREAM_LEAF_INSTRS ||
                b.d_params.bytes < ((size_t)s.banks[i].voices << s.banks[i].log2_p) * lp.k * sizeof(float) || (leaf_at + lp.ins.size()) * sizeof(LeafInstr) > strm.d_leaf.bytes)
                throw Error(FR_ERR_DEVICE, "internal: a leaf bank is not the plan's compiled bank");
            uint32_t result = lp.result;
            if (lp.result_kind == LEAF_IN) {                     // (a leaf that is a bare input: its row)
                size_t row = 0;
                const uint32_t slot = lp.result < lp.input_slots.size() ? lp.input_slots[lp.result] : UINT32_MAX;
                if (strm.now.store) { while (row < strm.now.streamed.size() && strm.now.streamed[row].slot != slot) ++row; }
                else row = (size_t)(std::find(s.input_slots.begin(), s.input_slots.end(), slot) - s.input_slots.begin());
                if (row >= l.n_rows) throw Error(FR_ERR_DEVICE, "internal: a streamed leaf reads a slot the stream does not feed");
                result = (uint32_t)row;
            }
            uint32_t result_kind = lp.result_kind;
            if (result_kind == LEAF_TRK || result_kind == LEAF_TRK_LIT) {   // (a leaf that is a bare track: its parked column)
                result = lp.track_index(result_kind, lp.result);
                result_kind = LEAF_TRK;
            }
            if (!lp.track_cols.empty()) {                        // FR_STREAM_TRACKS: the leaf's track columns
                if (lp.track_cols.size() > BANK_STREAM_LEAF_TRACKS || !s.has_tracks()) throw Error(FR_ERR_DEVICE, "internal: a leaf bank's tracks are not the plan's");
                StreamTrackArgs::Bank &tb = x.tr.bank[i];
                tb.n = (uint32_t)lp.track_cols.size();
                for (uint32_t q = 0; q < tb.n; ++q) {
                    tb.cols[q] = lp.track_cols[q].v;
                    if (lp.track_cols[q].literal) tb.literal |= 1u << q;
                }
            }
            x.l.mask |= 1u << i;
            x.l.bank[i] = {lp.ins.empty() ? nullptr : strm.d_leaf.as<uint4>() + leaf_at, (uint32_t)lp.ins.size(), lp.k, result_kind, result};
            leaf_at += lp.ins.size();
        }
        if (s.has_tracks()) {                                    // the staging as the device addresses it
            if (strm.h_trk.bytes < (size_t)s.track_rows * STREAM_BLOCK * sizeof(float)) throw Error(FR_ERR_DEVICE, "internal: the track staging does not hold the plan's rows");
            x.tr.staging = strm.h_trk.as_dev<float>();
            x.tr.first_slot = s.track_first;
            x.tr.rows = s.track_rows;
        }
    }
    // a stream that stores its rows: the buffers of the slots this launch appends to (streamstore.hpp StoreStreamed; the caller
    // has made room: stream_store_block_relaunches)
    if (strm.now.store) {
        if (strm.now.streamed.size() != l.n_rows || l.n_rows > BANK_STREAM_ROWS) throw Error(FR_ERR_DEVICE, "internal: the streamed slots are not the launch's rows");
        for (size_t j = 0; j < strm.now.streamed.size(); ++j) {
            const StoreStreamed &ss = strm.now.streamed[j];
            if (!ss.has_data) continue;
            const InSlot &in = slots[ss.slot];
            if (!in.fed || !in.buf.p || idx < in.base || idx - in.base + STREAM_BLOCK > in.cap || in.cap * sizeof(float) > in.buf.bytes)
                throw Error(FR_ERR_DEVICE, "internal: a streamed slot's buffer has no room for a block");
            x.s.row[j] = {in.buf.as<float>(), in.base};
        }
    }
    launch_resident(strm.now, x);
}

// The history of a stream that continues the input store: for each streamed row the hist_cap frames before idx as the store
// answers them -- 0.0 before a slot's base, below the floor, beyond its length and for a slot never fed.
void fr_renderer::fill_stream_history(uint64_t idx) {
    const StreamLaunch &l = strm.now.launch;
    if (!l.hist_cap) return;
    const size_t bytes = (size_t)l.n_rows * l.hist_cap * sizeof(float);
    if (bytes > strm.d_hist.bytes || strm.now.streamed.size() != l.n_rows) throw Error(FR_ERR_DEVICE, "internal: the input history does not hold the stream's look-back");
    HIP_CHECK(hipMemsetAsync(strm.d_hist.p, 0, bytes, stream));
    const uint64_t mask = l.hist_cap - 1;
    for (size_t j = 0; j < strm.now.streamed.size(); ++j) {
        const DevInput d = dev_input(strm.now.streamed[j].slot);
        if (!d.data) continue;
        const uint64_t lo = std::max(d.base, idx > l.hist_cap ? idx - l.hist_cap : 0), hi = std::min(d.len, idx);
        float *row = strm.d_hist.as<float>() + j * l.hist_cap;
        for (uint64_t t = lo; t < hi;) {                         // (at most two pieces: the ring wraps once)
            const uint64_t n = std::min(hi - t, l.hist_cap - (t & mask));
            HIP_CHECK(hipMemcpyAsync(row + (t & mask), d.data + (t - d.base), n * sizeof(float), hipMemcpyDeviceToDevice, stream));
            t += n;
        }
    }
}

// A stream that stores its rows (FR_STREAM_STORE), the block [idx, idx + n_times) with rows for the slots [0, rows_fed): the
// resident launch is (re)started at head = idx.  `seek`: the block does not continue the renderer's head -- the store is reset as
// store_inputs resets it.  A first launch and a seek bring the rings up to idx (bring_up_rings: a call of zero own frames) and
// fill the stream's history from the store; a relaunch -- room in a slot's buffer, a slot more -- finds both as the stopped launch
// left them (a slot more moves the history's rows: then it is filled again from the store, which holds what it held).
void fr_renderer::launch_store_stream(uint64_t idx, uint32_t rows_fed, bool seek) {
    HIP_CHECK(hipSetDevice(device));
    Stream::Open &o = strm.now;
    bool relaunch = o.launched && !seek;
    const uint32_t n_slots = o.slots;
    if (!plan_current(n_slots)) throw Error(FR_ERR_DEVICE, "internal: a stream outlived its plan");
    std::vector<uint32_t> row_slots;
    std::string why;
    // (refused before anything is touched: the launch goes on, everything streamed so far is in the store's books)
    if (!stream_store_slots(o.plan.input_slots, slots, rows_fed, row_slots, &why)) throw Error(FR_ERR_UNSUPPORTED, "block streaming (FR_STREAM_STORE): " + why);
    if (!stop_resident(true)) {                  // (the launch did not end as it should: what the rings hold is not known)
        plan.stage_valid = false;
        ring_table.valid = false;
        relaunch = false;
    }
    reap();
    if (seek) {
        stream_store_seek(slots, segs, n_vecs, idx);
        head = idx;                              // (the store is empty at idx from here on, whatever becomes of the block: a retry there continues it)
        o.rows_open = false;
        history_floor = 0;
        plan.stage_valid = false;                // whatever the rings hold, they do not hold a seek to idx
        ring_table.valid = false;
    }
    history_floor = store_floor(history_floor, keep_frames(), idx);
    stream_store_feed(slots, rows_fed, idx);
    for (uint32_t r = 0; r < rows_fed; ++r) make_room(slots[r], STREAM_BLOCK, stream);   // (a block's room, whatever this block's length)
    bool same = row_slots.size() == o.streamed.size();
    for (size_t j = 0; same && j < row_slots.size(); ++j) same = o.streamed[j].slot == row_slots[j];
    if (!same || o.launch.n_rows != row_slots.size()) {
        o.launch.n_rows = (uint32_t)row_slots.size();
        upload_stream_programs(o.plan, o.launch, row_slots, n_slots);
    }
    o.streamed.resize(row_slots.size());
    for (size_t j = 0; j < row_slots.size(); ++j) o.streamed[j] = {row_slots[j], row_slots[j] < rows_fed};
    // (a relaunch with the same rows: rings and history stand as the stopped launch left them.  With another set of rows the
    //  history's rows change places: it is filled again from the store, which holds what the history held)
    if (!relaunch) bring_up_rings(n_slots, idx, STREAM_BLOCK, stream);
    if (!relaunch || !same) fill_stream_history(idx);
    if (relaunch) ++o.relaunches;
    start_resident(idx, false);
}

namespace {

template <class F>
fr_status guarded(fr_renderer *r, F &&f, bool keeps_stream = false) {
    if (!r) return FR_ERR_INVALID_ARG;
    try {
        if (r->strm.open && !keeps_stream) r->end_stream();   // any other call first retires the resident launch
        f();
        r->last_error.clear();
        return FR_OK;
    } catch (const Error &e) {
        r->last_error = e.what();
        return e.code;
    } catch (const std::bad_alloc &) {
        r->last_error = "host out of memory";
        return FR_ERR_OUT_OF_MEMORY;
    } catch (const std::exception &e) {
        r->last_error = e.what();
        return FR_ERR_INVALID_ARG;
    }
}

void check_fill_args(const void *out, uint32_t n_slots, uint64_t n_times, const float *in_data,
                     const uint64_t *offs, uint32_t n_rows) {
    if (!out && n_slots != 0 && n_times != 0) throw Error(FR_ERR_INVALID_ARG, "null output buffer");
    if (n_rows && !offs) throw Error(FR_ERR_INVALID_ARG, "null row offsets");
    if (n_rows && offs[n_rows] > offs[0] && !in_data) throw Error(FR_ERR_INVALID_ARG, "null input data");
    if (n_slots && n_times > (1ull << 40) / n_slots) throw Error(FR_ERR_INVALID_ARG, "render range too large");
}

// ---- per-renderer options (friendship_render_ext.h) -------------------------------------------------------------------
// One row per switch; the environment and fr_renderer_create_with_options both go through it.  `env`: the lenient reading
// the variable has always had (atoi, clamping).  An option must be decimal digits in [lo, hi] -- with `set`, one of the
// values whose bits it has -- or `word`, which stands for `word_value`.  `apply` stores a value in the renderer; `given`:
// it came from the environment or an option, not from the default.
enum OptionSource : uint8_t { OPTION_DEFAULT, OPTION_ENV, OPTION_GIVEN };
enum OptionListing : uint8_t { UNLISTED, LISTED, LISTED_WHEN_SET };
struct Knob {
    const char *name;
    int64_t dflt, lo, hi;
    uint32_t set;
    const char *word;
    int64_t word_value;
    int64_t (*env)(const char *e);
    void (*apply)(fr_renderer &r, int64_t v, bool given);
    uint8_t listed = LISTED;   // in fr_options_json: always, never, or once the environment or an option set it
};

int64_t env_on(const char *e) { return e[0] != '0'; }
int64_t env_int(const char *e) { return std::atoi(e); }
int64_t env_long(const char *e) { return std::atoll(e); }
int64_t env_clamp(const char *e, int lo, int hi) { return std::min(hi, std::max(lo, std::atoi(e))); }
constexpr int64_t ENV_REFUSED = INT64_MIN;   // an `env` reading that makes create fail (resolve_options)
int64_t env_strict_track_history(const char *e);
int64_t env_strict_ring_keep(const char *e);
int64_t env_strict_stream_programs(const char *e);
int64_t env_strict_stream_bus(const char *e);
int64_t env_strict_stream_inputs(const char *e);
int64_t env_strict_stream_banks(const char *e);
int64_t env_strict_loop_tiles(const char *e);
int64_t env_strict_loop_dyn(const char *e);
int64_t env_strict_stream_loops(const char *e);
int64_t env_strict_stream_general(const char *e);
int64_t env_strict_stream_dyn(const char *e);
int64_t env_strict_stream_history(const char *e);
int64_t env_strict_stream_effects(const char *e);
int64_t env_strict_stream_store(const char *e);
int64_t env_strict_stream_taps(const char *e);
int64_t env_strict_stream_sweep(const char *e);
int64_t env_strict_stream_leaves(const char *e);
int64_t env_strict_stream_tracks(const char *e);
bool parse_option(const Knob &k, const char *s, int64_t &v);

const Knob kKnobs[] = {
    {"FR_JIT", 1, 0, 1, 0, nullptr, 0, env_on, [](fr_renderer &r, int64_t v, bool) { r.allow_jit = v != 0; }},
    {"FR_STAGE_JIT", 1, 0, 1, 0, "force", 2, [](const char *e) -> int64_t { return e[0] == '0' ? 0 : (e[0] == '1' ? 1 : 2); },
     [](fr_renderer &r, int64_t v, bool) { r.stage_jit_mode = (int)v; }},
    {"FR_JIT_FMA", 1, 0, 1, 0, nullptr, 0, env_on, [](fr_renderer &r, int64_t v, bool) { r.jit_fma = v != 0; }},
    {"FR_JIT_CHUNKS", 1, 0, 1, 0, nullptr, 0, env_on, [](fr_renderer &r, int64_t v, bool) { r.bank_tune.jit_chunks = v != 0; }},
    {"FR_JIT_CHUNK_TARGET", 0, 0, 1 << 24, 0, nullptr, 0, [](const char *e) -> int64_t { return std::max(1, std::atoi(e)); },
     [](fr_renderer &r, int64_t v, bool) { r.bank_tune.jit_chunk_target = (uint64_t)v; }},
    {"FR_BANK_TEMPLATE", 1, 0, 1, 0, nullptr, 0, env_on, [](fr_renderer &r, int64_t v, bool) { r.allow_template = v != 0; }},
    {"FR_BANK_LEAF", 1, 0, 1, 0, nullptr, 0, [](const char *e) -> int64_t { return e[0] == '1'; },
     [](fr_renderer &r, int64_t v, bool) { r.bank_tune.leaf_variant = v ? 1u : 0u; }},
    {"FR_BANK_MULTI", 1, 0, 1, 0, nullptr, 0, env_on, [](fr_renderer &r, int64_t v, bool) { r.bank_tune.multi = v != 0; }},
    {"FR_BANK_SHORT", 1, 0, 1, 0, nullptr, 0, env_on, [](fr_renderer &r, int64_t v, bool) { r.bank_tune.short_kernel = v != 0; }},
    {"FR_SHORT_PAIRS", 1000, 0, 1 << 30, 0, nullptr, 0, env_int, [](fr_renderer &r, int64_t v, bool) { r.bank_tune.short_pairs = (uint64_t)v; }},
    {"FR_SHORT_WGS", 0, 0, 1 << 30, 0, nullptr, 0, env_int, [](fr_renderer &r, int64_t v, bool) { r.bank_tune.short_wgs = (uint64_t)v; }},
    {"FR_SHORT_NW", 0, 0, 16, 1u << 0 | 1u << 4 | 1u << 8 | 1u << 16, nullptr, 0, env_int,
     [](fr_renderer &r, int64_t v, bool) { r.bank_tune.short_nw = (uint32_t)v; }},
    {"FR_BANK_NW", 0, 0, 8, 1u << 0 | 1u << 4 | 1u << 8, nullptr, 0, env_int, [](fr_renderer &r, int64_t v, bool) { r.bank_tune.bank_nw = (uint32_t)v; }},
    {"FR_BANK_F", 0, 0, 4, 1u << 0 | 1u << 1 | 1u << 2 | 1u << 4, nullptr, 0, env_int,
     [](fr_renderer &r, int64_t v, bool) { r.bank_tune.bank_f = (uint32_t)v; }},
    {"FR_HOST_MAPPED", 2, 0, 3, 0, nullptr, 0, env_int, [](fr_renderer &r, int64_t v, bool) {
         r.host_out_mapped = (v & 1) != 0;
         r.host_rows_mapped = (v & 2) != 0;
     }},
    {"FR_HOST_STREAM", 1, 0, 1, 0, nullptr, 0, env_on, [](fr_renderer &r, int64_t v, bool) { r.host_stream = v != 0; }},
    {"FR_HOST_SMALL_KB", 96, 0, 1 << 20, 0, nullptr, 0, [](const char *e) -> int64_t { return std::max(0, std::atoi(e)); },
     [](fr_renderer &r, int64_t v, bool) { r.host_small_bytes = (size_t)v << 10; }},
    {"FR_HOST_DIRECT", 1, 0, 1, 0, nullptr, 0, env_on, [](fr_renderer &r, int64_t v, bool) { r.host_direct = v != 0; }},
    {"FR_STREAM_IDLE_MS", BANK_STREAM_IDLE_MS, 1, 60000, 0, nullptr, 0, [](const char *e) { return env_clamp(e, 1, 60000); },
     [](fr_renderer &r, int64_t v, bool) { r.stream_idle_ms = (uint32_t)v; }},
    {"FR_STAGE_STRIDED", 1, 0, 1, 0, nullptr, 0, env_on, [](fr_renderer &r, int64_t v, bool) { r.fused_strided_ok = v != 0; }},
    {"FR_STAGE_BLOCK", 0, 0, 16, 0, nullptr, 0, [](const char *e) -> int64_t { return std::max(0, std::atoi(e)); },
     [](fr_renderer &r, int64_t v, bool) { r.stage_block_env = (uint32_t)v; }},
    // (setting either exchange knob also tiles over the host-callback transport)
    {"FR_EXCHANGE_TILES", 4, 1, 64, 0, nullptr, 0, [](const char *e) { return env_clamp(e, 1, 64); }, [](fr_renderer &r, int64_t v, bool given) {
         r.x_max_tiles = (uint32_t)v;
         r.x_tiles_explicit = r.x_tiles_explicit || given;
     }},
    {"FR_EXCHANGE_MIN_TILE", 1024, 64, 1 << 20, 0, nullptr, 0, [](const char *e) { return env_clamp(e, 64, 1 << 20); },
     [](fr_renderer &r, int64_t v, bool given) {
         r.x_min_tile = (uint32_t)v;
         r.x_tiles_explicit = r.x_tiles_explicit || given;
     }},
    // (the helper threads are a process-wide pool; how many of them a renderer's lowering uses is its own)
    {"FR_LOWER_THREADS", (int64_t)default_lowering_threads(), 1, 1024, 0, nullptr, 0, [](const char *e) -> int64_t { return std::max(1, std::atoi(e)); },
     [](fr_renderer &r, int64_t v, bool) { r.lower_threads = (unsigned)v; }},
    {"FR_LOWER_PAR_MIN_NODES", 200000, 0, 1ll << 40, 0, nullptr, 0, env_long, [](fr_renderer &r, int64_t v, bool) { r.lower_min_nodes = (size_t)v; }},
    {"FR_LOWER_PAR_MIN_EDIT", 16384, 0, 1ll << 40, 0, nullptr, 0, env_long, [](fr_renderer &r, int64_t v, bool) { r.lower_min_edit = (size_t)v; }},
    // Rendering modes rather than tuning: fr_plan_json reports them (delay_observed, delay_observed_max), fr_options_json lists
    // the tuning switches only
    {"FR_DELAY_OBSERVED", 0, 0, 1, 0, nullptr, 0, env_on, [](fr_renderer &r, int64_t v, bool) { r.delay_observed = v != 0; }, false},
    {"FR_DELAY_OBSERVED_MAX", 1 << 20, 1024, 1 << 28, 0, nullptr, 0, [](const char *e) { return env_clamp(e, 1024, 1 << 28); },
     [](fr_renderer &r, int64_t v, bool) { r.delay_observed_max = (uint64_t)v; }, false},
    // Track history (frames of every track row kept on the device; 0 = tracks are readable by voice leaves of their own call
    // only).  The environment is read as strictly as an option: a value the table refuses makes create fail.  A rendering
    // mode too (fr_plan_json: track_history), listed by fr_options_json once it is set.
    {"FR_TRACK_HISTORY", 0, 0, 1 << 24, 0, nullptr, 0, env_strict_track_history,
     [](fr_renderer &r, int64_t v, bool) {
         r.track_history = (uint64_t)v;
         uint64_t cap = 64;
         while (cap < r.track_history) cap <<= 1;
         r.tail_cap = v ? cap : 0;
     }, LISTED_WHEN_SET},
    // Kept delay lines: a re-plan keeps the rings an edit cannot have changed (fr_plan_json: ring_keep, ring_state).  Strict
    // like FR_TRACK_HISTORY, and listed once set.
    {"FR_RING_KEEP", 0, 0, 1, 0, nullptr, 0, env_strict_ring_keep, [](fr_renderer &r, int64_t v, bool) { r.ring_keep = v != 0; }, LISTED_WHEN_SET},
    // Block streaming of plans with stage programs and rings behind one voice bank (streamplan.hpp; fr_plan_json: stream).
    // Strict and listed once set, like the two above.
    {"FR_STREAM_PROGRAMS", 0, 0, 1, 0, nullptr, 0, env_strict_stream_programs, [](fr_renderer &r, int64_t v, bool) { r.stream_programs = v != 0; }, LISTED_WHEN_SET},
    // Mix-bus programs across voices in block streaming (streamplan.hpp StreamEnv::bus; fr_plan_json: stream.bus_programs).
    // Inert without FR_STREAM_PROGRAMS.  Strict and listed once set.
    {"FR_STREAM_BUS", 0, 0, 1, 0, nullptr, 0, env_strict_stream_bus, [](fr_renderer &r, int64_t v, bool) { r.stream_bus = v != 0; }, LISTED_WHEN_SET},
    // Control rows in block streaming: programs read up to STREAM_MAX_INPUTS input slots at the current frame (streamplan.hpp
    // StreamEnv::inputs; fr_stream_block_rows; fr_plan_json: stream.input_slots).  Inert without FR_STREAM_PROGRAMS.  Strict and
    // listed once set.
    {"FR_STREAM_INPUTS", 0, 0, 1, 0, nullptr, 0, env_strict_stream_inputs, [](fr_renderer &r, int64_t v, bool) { r.stream_inputs = v != 0; }, LISTED_WHEN_SET},
    // Voices of several banks in block streaming: 2..STREAM_MAX_BANKS bank launches -- several partial counts, voices to rows
    // next to voices behind programs -- in one resident launch (streamplan.hpp StreamEnv::banks; fr_plan_json: stream.banks).
    // Inert without FR_STREAM_PROGRAMS.  Strict and listed once set.
    {"FR_STREAM_BANKS", 0, 0, 1, 0, nullptr, 0, env_strict_stream_banks, [](fr_renderer &r, int64_t v, bool) { r.stream_banks = v != 0; }, LISTED_WHEN_SET},
    // Loop tiles: the strided launches of feedback plans whose stride is at most LOOP_TILE_MAX_STRIDE frames stage a tile of frames
    // in LDS (callplan.hpp loop_tile; fr_plan_json: loop_tiles, the launches' +tile).  Same bits.  Strict and listed once set.
    {"FR_LOOP_TILES", 0, 0, 1, 0, nullptr, 0, env_strict_loop_tiles, [](fr_renderer &r, int64_t v, bool given) {
         r.loop_tiles = v != 0;
         r.loop_tiles_given = given;
     }, LISTED_WHEN_SET},
    // Feedback loops shorter than a block in block streaming -- a one-pole filter, a short comb, a 32-frame bus echo -- and the
    // taps behind them (streamplan.hpp StreamEnv::loops; fr_plan_json: stream.loop_programs).  Inert without FR_STREAM_PROGRAMS.
    // Strict and listed once set.
    {"FR_STREAM_LOOPS", 0, 0, 1, 0, nullptr, 0, env_strict_stream_loops, [](fr_renderer &r, int64_t v, bool) { r.stream_loops = v != 0; }, LISTED_WHEN_SET},
    // Voices of any partial count in block streaming: general voices (items plus a merge schedule) and balanced voices of 32 or
    // 64 partials, one workgroup per voice (streamplan.hpp StreamEnv::general; fr_plan_json: stream.general_voices).  Inert
    // without FR_STREAM_PROGRAMS.  Strict and listed once set.
    {"FR_STREAM_GENERAL", 0, 0, 1, 0, nullptr, 0, env_strict_stream_general, [](fr_renderer &r, int64_t v, bool) { r.stream_general = v != 0; }, LISTED_WHEN_SET},
    // Delays of a voice by a signal amount in block streaming -- a chorus, a flanger, a vibrato, a delay time on a knob
    // (streamplan.hpp StreamEnv::dyn; fr_plan_json: stream.dyn_reads).  Inert without FR_STREAM_PROGRAMS.  Strict and listed once set.
    {"FR_STREAM_DYN", 0, 0, 1, 0, nullptr, 0, env_strict_stream_dyn, [](fr_renderer &r, int64_t v, bool) { r.stream_dyn = v != 0; }, LISTED_WHEN_SET},
    // Delayed reads of input rows in block streaming -- a pre-delay on a control row, a delayed gate, Delay(In(0), d); with
    // FR_STREAM_DYN by a signal amount -- from a history of the streamed rows (streamplan.hpp StreamEnv::history; fr_plan_json:
    // stream.hist_reads, stream.input_lookback).  Inert without FR_STREAM_PROGRAMS.  Strict and listed once set.
    {"FR_STREAM_HISTORY", 0, 0, 1, 0, nullptr, 0, env_strict_stream_history, [](fr_renderer &r, int64_t v, bool) { r.stream_history = v != 0; }, LISTED_WHEN_SET},
    // Patches without a voice in block streaming -- an echo, a comb or a flanger on a row the host feeds in, a gain on a control
    // row, a one-pole smoother on a knob: the programs are dealt over segments, one wave each (streamplan.hpp StreamEnv::effects;
    // fr_plan_json: stream.segments).  Inert without FR_STREAM_PROGRAMS.  Strict and listed once set.
    {"FR_STREAM_EFFECTS", 0, 0, 1, 0, nullptr, 0, env_strict_stream_effects, [](fr_renderer &r, int64_t v, bool) { r.stream_effects = v != 0; }, LISTED_WHEN_SET},
    // A stream that survives edits: the resident launch appends the rows it is fed to the input store, a stream's first block
    // continues the renderer's head instead of seeking, and closing a stream leaves the renderer as an ordinary call would
    // (streamstore.hpp; fr_plan_json: stream.store).  Inert without FR_STREAM_PROGRAMS, with FR_DELAY_OBSERVED=1 and with declared
    // track slots.  Strict and listed once set.
    {"FR_STREAM_STORE", 0, 0, 1, 0, nullptr, 0, env_strict_stream_store, [](fr_renderer &r, int64_t v, bool) { r.stream_store = v != 0; }, LISTED_WHEN_SET},
    // Short and signal delays of computed values in block streaming -- a two-tap FIR behind an envelope, a chorus behind the ADSR or
    // on the mix bus: a plan without feedback and without a fused form is served in its level form, a reader below a block follows
    // its storer (streamplan.hpp StreamEnv::taps; fr_plan_json: stream.levels, stream.short_reads, stream.dyn_ring_reads).  Inert
    // without FR_STREAM_PROGRAMS.  Strict and listed once set.
    {"FR_STREAM_TAPS", 0, 0, 1, 0, nullptr, 0, env_strict_stream_taps, [](fr_renderer &r, int64_t v, bool) { r.stream_taps = v != 0; }, LISTED_WHEN_SET},
    // Feedback through a Delay of a signal amount -- a flanger with regeneration, a comb with vibrato, a tape echo whose time
    // wobbles: a loop with no constant Delay on it is cut at its Delay of a signal amount when the amount is proven >= 1 frame and
    // never NaN, and its plan runs W frames at a time: 1 = on stage_sweep_kernel, 2 = on stage_kernel, a launch per W frames
    // (callplan.hpp loop_sweep; fr_plan_json: loop_dyn, the launches' +sweep and /windows).  Strict and listed once set.
    {"FR_LOOP_DYN", 0, 0, 2, 0, nullptr, 0, env_strict_loop_dyn, [](fr_renderer &r, int64_t v, bool given) {
         r.loop_dyn = (int)v;
         r.loop_dyn_given = given;
     }, LISTED_WHEN_SET},
    // Delays by a signal amount inside feedback loops shorter than a block in block streaming -- a flanger with regeneration, a comb
    // with vibrato (a sweep plan, FR_LOOP_DYN), a chorus into a comb, a signal tap behind a loop: a loop program walks the block in
    // sweeps of its width (streamplan.hpp StreamEnv::sweep; fr_plan_json: stream.sweep_programs).  Acts on top of FR_STREAM_PROGRAMS,
    // FR_STREAM_LOOPS and FR_STREAM_DYN; inert without them.  Strict and listed once set.
    {"FR_STREAM_SWEEP", 0, 0, 1, 0, nullptr, 0, env_strict_stream_sweep, [](fr_renderer &r, int64_t v, bool) { r.stream_sweep = v != 0; }, LISTED_WHEN_SET},
    // Compiled voices in block streaming -- voices whose leaves are not the sine partial but share one expression shape: a triangle
    // partial, a partial times a control row, a sawtooth with a divisor: a leaf bank, whose leaf the rendering waves interpret as a
    // register program (leafprog.hpp; streamplan.hpp StreamEnv::leaves; fr_plan_json: stream.leaf_banks).  Inert without
    // FR_STREAM_PROGRAMS.  Strict and listed once set.
    {"FR_STREAM_LEAVES", 0, 0, 1, 0, nullptr, 0, env_strict_stream_leaves, [](fr_renderer &r, int64_t v, bool) { r.stream_leaves = v != 0; }, LISTED_WHEN_SET},
    // Track voices in block streaming -- compiled voices whose leaves read per-partial track rows (fr_set_track_inputs): a leaf bank
    // whose program has track operands, the block's matrix (fr_stream_block_dense) staged in mapped pinned memory (streamplan.hpp
    // StreamEnv::tracks; fr_plan_json: stream.tracks).  Inert without FR_STREAM_PROGRAMS and FR_STREAM_LEAVES.  Strict and listed once set.
    {"FR_STREAM_TRACKS", 0, 0, 1, 0, nullptr, 0, env_strict_stream_tracks, [](fr_renderer &r, int64_t v, bool) { r.stream_tracks = v != 0; }, LISTED_WHEN_SET},
};
static_assert(sizeof kKnobs / sizeof kKnobs[0] == N_OPTIONS, "N_OPTIONS counts the rows of kKnobs");

static int64_t env_strict(const char *name, const char *e) {
    int64_t v = 0;
    for (const Knob &k : kKnobs)
        if (std::strcmp(k.name, name) == 0) return parse_option(k, e, v) ? v : ENV_REFUSED;
    return ENV_REFUSED;
}
int64_t env_strict_track_history(const char *e) { return env_strict("FR_TRACK_HISTORY", e); }
int64_t env_strict_ring_keep(const char *e) { return env_strict("FR_RING_KEEP", e); }
int64_t env_strict_stream_programs(const char *e) { return env_strict("FR_STREAM_PROGRAMS", e); }
int64_t env_strict_stream_bus(const char *e) { return env_strict("FR_STREAM_BUS", e); }
int64_t env_strict_stream_inputs(const char *e) { return env_strict("FR_STREAM_INPUTS", e); }
int64_t env_strict_stream_banks(const char *e) { return env_strict("FR_STREAM_BANKS", e); }
int64_t env_strict_loop_tiles(const char *e) { return env_strict("FR_LOOP_TILES", e); }
int64_t env_strict_loop_dyn(const char *e) { return env_strict("FR_LOOP_DYN", e); }
int64_t env_strict_stream_loops(const char *e) { return env_strict("FR_STREAM_LOOPS", e); }
int64_t env_strict_stream_general(const char *e) { return env_strict("FR_STREAM_GENERAL", e); }
int64_t env_strict_stream_dyn(const char *e) { return env_strict("FR_STREAM_DYN", e); }
int64_t env_strict_stream_history(const char *e) { return env_strict("FR_STREAM_HISTORY", e); }
int64_t env_strict_stream_effects(const char *e) { return env_strict("FR_STREAM_EFFECTS", e); }
int64_t env_strict_stream_store(const char *e) { return env_strict("FR_STREAM_STORE", e); }
int64_t env_strict_stream_taps(const char *e) { return env_strict("FR_STREAM_TAPS", e); }
int64_t env_strict_stream_sweep(const char *e) { return env_strict("FR_STREAM_SWEEP", e); }
int64_t env_strict_stream_leaves(const char *e) { return env_strict("FR_STREAM_LEAVES", e); }
int64_t env_strict_stream_tracks(const char *e) { return env_strict("FR_STREAM_TRACKS", e); }

bool parse_option(const Knob &k, const char *s, int64_t &v) {
    if (k.word && std::strcmp(s, k.word) == 0) {
        v = k.word_value;
        return true;
    }
    const size_t n = std::strlen(s);
    if (n == 0 || n > 15) return false;   // (15 digits cannot overflow an int64_t)
    v = 0;
    for (size_t i = 0; i < n; ++i) {
        if (s[i] < '0' || s[i] > '9') return false;
        v = v * 10 + (s[i] - '0');
    }
    if (v < k.lo || v > k.hi) return false;
    return !k.set || (v < 32 && ((k.set >> v) & 1u));
}

std::string option_text(const Knob &k, int64_t v) { return k.word && v == k.word_value ? std::string(k.word) : std::to_string(v); }

// Every knob's value and source: the default, then the environment, then the options.  False (nothing resolved) for an
// option the table refuses.
bool resolve_options(const fr_option *options, size_t n_options, int64_t *value, uint8_t *source) {
    if (n_options && !options) return false;
    for (size_t i = 0; i < N_OPTIONS; ++i) {
        value[i] = kKnobs[i].dflt;
        source[i] = OPTION_DEFAULT;
        if (const char *e = std::getenv(kKnobs[i].name)) {
            value[i] = kKnobs[i].env(e);
            if (value[i] == ENV_REFUSED) return false;
            source[i] = OPTION_ENV;
        }
    }
    for (size_t j = 0; j < n_options; ++j) {
        const fr_option &o = options[j];
        if (!o.name || !o.value) return false;
        size_t i = 0;
        while (i < N_OPTIONS && std::strcmp(o.name, kKnobs[i].name) != 0) ++i;
        // (not in the table: unknown, or process-wide -- FR_JIT_CACHE, FR_JIT_DUMP, FR_HOST_TRACE, FR_LOWER_TRACE, FR_PLAN_TRACE
        //  and FR_LOWER_HUGEPAGES act on the process: files, stderr, the memory allocator)
        if (i == N_OPTIONS) return false;
        if (source[i] == OPTION_GIVEN || !parse_option(kKnobs[i], o.value, value[i])) return false;
        source[i] = OPTION_GIVEN;
    }
    return true;
}

}  // namespace

extern "C" {

fr_status fr_renderer_create(const fr_config *cfg, fr_renderer **out) { return fr_renderer_create_with_options(cfg, nullptr, 0, out); }

fr_status fr_renderer_create_with_options(const fr_config *cfg, const fr_option *options, size_t n_options, fr_renderer **out) {
    if (!out) return FR_ERR_INVALID_ARG;
    *out = nullptr;
    if (cfg && cfg->abi_version != FR_ABI_VERSION) return FR_ERR_INVALID_ARG;
    int64_t opt_value[N_OPTIONS];
    uint8_t opt_source[N_OPTIONS];
    if (!resolve_options(options, n_options, opt_value, opt_source)) return FR_ERR_INVALID_ARG;
    int mode = cfg ? cfg->mode : FR_MODE_AUTO;
    if (mode < FR_MODE_AUTO || mode > FR_MODE_STAGED) return FR_ERR_INVALID_ARG;
    if (cfg && ((cfg->flags & ~FR_CONFIG_SYNC_COMPILE) != 0 || cfg->reserved != 0)) return FR_ERR_INVALID_ARG;
    if (cfg && cfg->semantics != FR_SEMANTICS_REFERENCE && cfg->semantics != FR_SEMANTICS_SPARKLE) return FR_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return FR_ERR_NO_DEVICE;
    int dev = cfg ? cfg->device : -1;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) return FR_ERR_NO_DEVICE;
    }
    if (dev >= ndev) return FR_ERR_INVALID_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return FR_ERR_NO_DEVICE;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FR_ERR_NO_DEVICE;   // code objects are gfx950 only
    if (hipSetDevice(dev) != hipSuccess) return FR_ERR_NO_DEVICE;
    fr_renderer *r = new (std::nothrow) fr_renderer();
    if (!r) return FR_ERR_OUT_OF_MEMORY;
    // The first C++ exception a process throws makes the unwinder walk every loaded object's unwind tables (under the
    // loader's lock: other throwing threads queue behind it) -- 82 ms measured inside a fill_buffer call with the HIP
    // runtime and hipRTC loaded.  The engine uses exceptions on rare paths of a call (a lowering thread handing its sub-tree
    // to the sequential pass, a program a compiled kernel cannot take); pay for the walk here instead.
    try { throw Error(FR_OK, ""); } catch (const Error &) {}
    r->device = dev;
    r->mode = mode;
    r->jit_async_configured = !(cfg && (cfg->flags & FR_CONFIG_SYNC_COMPILE));
    r->jit_cache.set_async(r->jit_async_configured);
    r->jit_cache.set_sparkle(cfg && cfg->semantics == FR_SEMANTICS_SPARKLE);
    r->mirror.sparkle = cfg && cfg->semantics == FR_SEMANTICS_SPARKLE;
    r->semantics = cfg ? cfg->semantics : FR_SEMANTICS_REFERENCE;
    r->history_frames = cfg ? cfg->history_frames : 0;
    for (size_t i = 0; i < N_OPTIONS; ++i) {
        kKnobs[i].apply(*r, opt_value[i], opt_source[i] != OPTION_DEFAULT);
        r->option_value[i] = opt_value[i];
        r->option_source[i] = opt_source[i];
    }
    r->jit_cache.set_fma_fold(r->jit_fma);
    r->lowering.set_parallel(r->lower_threads, r->lower_min_nodes, r->lower_min_edit);
    if (const char *tv2 = std::getenv("FR_HOST_TRACE")) r->host_trace = tv2[0] == '1';   // (process-wide switches: environment only)
    r->device_cus = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) != hipSuccess) {
        delete r;
        return FR_ERR_DEVICE;
    }
    *out = r;
    return FR_OK;
}

void fr_renderer_destroy(fr_renderer *r) { delete r; }

fr_status fr_on_add_node(fr_renderer *r, uint32_t handle, const fr_effect *effect) {
    return guarded(r, [&] { r->mirror.add_node(handle, effect); });
}
fr_status fr_on_del_node(fr_renderer *r, uint32_t handle) {
    return guarded(r, [&] { r->mirror.del_node(handle); });
}
fr_status fr_on_add_edge(fr_renderer *r, const fr_edge *edge) {
    return guarded(r, [&] {
        if (!edge) throw Error(FR_ERR_INVALID_ARG, "null edge");
        r->mirror.add_edge(*edge);
    });
}
fr_status fr_on_del_edge(fr_renderer *r, const fr_edge *edge) {
    return guarded(r, [&] {
        if (!edge) throw Error(FR_ERR_INVALID_ARG, "null edge");
        r->mirror.del_edge(*edge);
    });
}
fr_status fr_on_add_nodes(fr_renderer *r, const uint32_t *handles, const fr_effect *const *effects, size_t n) {
    return guarded(r, [&] {
        if (n && (!handles || !effects)) throw Error(FR_ERR_INVALID_ARG, "null array");
        r->mirror.nodes.reserve(r->mirror.nodes.size() + n);
        for (size_t i = 0; i < n; ++i) r->mirror.add_node(handles[i], effects[i]);
    });
}
fr_status fr_on_add_edges(fr_renderer *r, const fr_edge *edges, size_t n) {
    return guarded(r, [&] {
        if (n && !edges) throw Error(FR_ERR_INVALID_ARG, "null array");
        for (size_t i = 0; i < n; ++i) r->mirror.add_edge(edges[i]);
    });
}

fr_status fr_fill_buffer(fr_renderer *r, float *out, uint32_t n_slots, uint64_t n_times, uint64_t idx,
                         const float *in_data, const uint64_t *in_row_offsets, uint32_t n_in_rows) {
    return guarded(r, [&] {
        check_fill_args(out, n_slots, n_times, in_data, in_row_offsets, n_in_rows);
        HIP_CHECK(hipSetDevice(r->device));
        hipStream_t st = r->stream;
        r->order_after_previous(st);
        r->ensure_plan(n_slots, st);           // graph errors surface before the input store is touched
        const auto snap = r->snapshot_store(idx);
        try {
        r->store_inputs(n_slots, n_times, idx, in_data, in_row_offsets, n_in_rows, false, st);
        size_t bytes = (size_t)n_slots * n_times * sizeof(float);
        // (Rendering a long call as 2-4 sub-calls so that chunk c's D2H overlaps chunk c+1's kernels was tried: every
        //  extra sub-call costs ~35 us of launch/sync overhead and smaller, less efficient launches -- 197 us became
        //  231 / 242 / 277 us at 2 / 3 / 4 chunks for config C; profiles/r01_host_path.txt.)
        // sharded: only the rows this rank owns come back (rank 0 under FR_SHARD_GATHER: every row)
        uint32_t row_lo, row_hi;
        r->my_rows(n_slots, row_lo, row_hi);
        const bool gather = r->sharded() && (r->shard_flags & FR_SHARD_GATHER);
        // (Pipelining the call -- row groups chained over a copy stream with events, or two halves on two streams of
        //  different priority -- was measured and is slower: every cross-stream hand-off costs tens of microseconds on this
        //  stack, profiles/r02_host_path.txt.  What helps is not moving bytes twice.)
        using clk = std::chrono::steady_clock;
        const auto t_a = clk::now();
        // A destination the host has page-locked (fr_host_register) is written by the kernels themselves: no copy of the
        // 1.2 MB at all (the launch runs ~19 us longer for its stores crossing PCIe, against ~40 us of D2H).
        float *direct = nullptr;
        if (!gather && bytes && r->host_direct)
            for (const auto &rg : r->registered)
                if ((char *)out >= rg.first && (char *)out + bytes <= rg.first + rg.second) {
                    void *dp = nullptr;
                    if (hipHostGetDevicePointer(&dp, out, 0) == hipSuccess) direct = (float *)dp;
                    else (void)hipGetLastError();
                    break;
                }
        if (direct) {
            r->execute(direct, n_slots, n_times, idx, st);
            HIP_CHECK(hipStreamSynchronize(st));   // synchronous contract: dispatch.rs:150-151
        } else if (bytes >= (256u << 10) && r->can_stream_rows(n_slots, n_times)) {   // (below that one D2H is as quick)
            // Streamed: rows are copied to the caller's buffer as their flags arrive, under the rest of the launch.
            r->h_out_stage.ensure(bytes);
            if ((size_t)n_slots * sizeof(uint32_t) > r->h_row_flags.bytes) {
                r->h_row_flags.ensure((size_t)n_slots * 2 * sizeof(uint32_t));
                std::memset(r->h_row_flags.p, 0, r->h_row_flags.bytes);
                r->host_seq = 0;
            }
            r->clean_counters(st);
            if ((size_t)n_slots * sizeof(uint32_t) > r->d_row_done.bytes) {
                r->d_row_done.ensure((size_t)n_slots * 2 * sizeof(uint32_t));
                HIP_CHECK(hipMemsetAsync(r->d_row_done.p, 0, r->d_row_done.bytes, st));
            }
            if (++r->host_seq == 0) {   // (wrapped: flags restart from a clean slate)
                std::memset(r->h_row_flags.p, 0, r->h_row_flags.bytes);
                r->host_seq = 1;
            }
            const uint32_t seq = r->host_seq;
            r->flag_out.host_flags = r->h_row_flags.as_dev<uint32_t>();
            r->flag_out.row_done = r->d_row_done.as<uint32_t>();
            r->flag_out.value = seq;
            struct Clear { fr_renderer *r; ~Clear() { r->flag_out = fr_renderer::FlagOut{}; } } clear{r};
            r->execute(r->h_out_stage.as_dev<float>(), n_slots, n_times, idx, st);
            const uint32_t *flags = r->h_row_flags.as<uint32_t>();
            const float *stage = r->h_out_stage.as<float>();
            r->stream_pending.resize(n_slots);
            for (uint32_t i = 0; i < n_slots; ++i) r->stream_pending[i] = i;
            size_t left = n_slots;
            uint64_t idle = 0;
            while (left) {
                bool progress = false;
                for (size_t i = 0; i < left;) {
                    const uint32_t row = r->stream_pending[i];
                    if (__atomic_load_n(flags + row, __ATOMIC_ACQUIRE) == seq) {
                        std::memcpy(out + (size_t)row * n_times, stage + (size_t)row * n_times, n_times * sizeof(float));
                        r->stream_pending[i] = r->stream_pending[--left];
                        progress = true;
                    } else {
                        ++i;
                    }
                }
                if (!progress && (++idle & 0xFFFFu) == 0 && hipStreamQuery(st) != hipErrorNotReady) {
                    // the launch is over (or failed) and a flag never came: report rather than spin for ever
                    HIP_CHECK(hipStreamSynchronize(st));
                    for (size_t i = 0; i < left; ++i)
                        if (__atomic_load_n(flags + r->stream_pending[i], __ATOMIC_ACQUIRE) != seq)
                            throw Error(FR_ERR_DEVICE, "internal: a rendered row was never published to the host");
                }
            }
            HIP_CHECK(hipStreamSynchronize(st));   // (everything is done; this only retires the launch)
        } else if ((r->host_out_mapped || bytes <= r->host_small_bytes) && !gather) {
            // small results (a real-time block: 64 frames x 64 voices = 16 KB): the kernels store straight into mapped pinned
            // memory and the host copies the few KB itself -- a D2H copy costs ~12 us of launch latency more than it moves
            // (64-frame call at config C: 35 -> 23 us, tools/host_short_probe.py); large results pay for it in cold CPU reads
            // kernels store finished frames straight into mapped pinned memory; one wait, one copy to the caller's buffer
            r->h_out_stage.ensure(bytes);
            r->execute(r->h_out_stage.as_dev<float>(), n_slots, n_times, idx, st);
            const auto t_b = clk::now();
            HIP_CHECK(hipStreamSynchronize(st));   // synchronous contract: dispatch.rs:150-151
            const auto t_c = clk::now();
            const size_t off = (size_t)row_lo * n_times, cnt = (size_t)(row_hi - row_lo) * n_times;
            if (cnt) std::memcpy(out + off, r->h_out_stage.as<float>() + off, cnt * sizeof(float));
            if (r->host_trace) {
                r->trace_us[0] += std::chrono::duration<double, std::micro>(t_b - t_a).count();
                r->trace_us[1] += std::chrono::duration<double, std::micro>(t_c - t_b).count();
                r->trace_us[2] += std::chrono::duration<double, std::micro>(clk::now() - t_c).count();
                ++r->trace_n;
            }
        } else {
            r->d_out.ensure(bytes);
            r->execute(r->d_out.as<float>(), n_slots, n_times, idx, st);
            if (gather) {
                r->gather_rows(r->d_out.as<float>(), n_slots, n_times, st);
                if (r->shard.rank == 0) { row_lo = 0; row_hi = n_slots; }
            }
            const size_t off = (size_t)row_lo * n_times, cnt = (size_t)(row_hi - row_lo) * n_times;
            const auto t_b = clk::now();
            if (cnt) HIP_CHECK(hipMemcpyAsync(out + off, r->d_out.as<float>() + off, cnt * sizeof(float), hipMemcpyDeviceToHost, st));
            const auto t_c = clk::now();
            HIP_CHECK(hipStreamSynchronize(st));
            if (r->host_trace) {
                r->trace_us[0] += std::chrono::duration<double, std::micro>(t_b - t_a).count();
                r->trace_us[1] += std::chrono::duration<double, std::micro>(t_c - t_b).count();
                r->trace_us[2] += std::chrono::duration<double, std::micro>(clk::now() - t_c).count();
                ++r->trace_n;
            }
        }
        } catch (...) {
            r->rollback_store(snap);
            throw;
        }
        r->last_pending = false;               // everything issued so far, on any stream, is complete (order_after_previous)
        r->head = idx + n_times;               // reference.rs:84
    });
}

fr_status fr_fill_buffer_device(fr_renderer *r, float *d_out, uint32_t n_slots, uint64_t n_times, uint64_t idx,
                                const float *d_in_data, const uint64_t *in_row_offsets, uint32_t n_in_rows,
                                void *stream) {
    return guarded(r, [&] {
        check_fill_args(d_out, n_slots, n_times, d_in_data, in_row_offsets, n_in_rows);
        HIP_CHECK(hipSetDevice(r->device));
        hipStream_t st = (hipStream_t)stream;
        // Independent of the previous call (may overlap with it on another stream): a plan without state, no seek, no new
        // plan, and every row full length -- padding a short row reads the slot's last stored sample, which the previous
        // call may still be writing.
        bool independent = r->plan_is_stateless(n_slots) && idx == r->head;
        for (uint32_t i = 0; independent && i < n_in_rows; ++i) independent = in_row_offsets[i + 1] - in_row_offsets[i] == n_times;
        r->host_pipelines = independent && r->last_pending && r->last_stream != st;
        struct Reset { fr_renderer *r; ~Reset() { r->host_pipelines = false; } } reset{r};
        r->order_after_previous(st, independent);
        r->used_scratch = false;
        r->ensure_plan(n_slots, st);
        const auto snap = r->snapshot_store(idx);
        try {
            r->store_inputs(n_slots, n_times, idx, d_in_data, in_row_offsets, n_in_rows, true, st);
            r->execute(d_out, n_slots, n_times, idx, st);
            r->gather_rows(d_out, n_slots, n_times, st);
        } catch (...) {
            r->rollback_store(snap);
            throw;
        }
        r->remember_async(st, independent && !r->used_scratch);
        r->head = idx + n_times;
    });
}

fr_status fr_set_track_inputs(fr_renderer *r, uint32_t first_slot) {
    return guarded(r, [&] {
        if (r->track_from == first_slot) return;
        r->track_from = first_slot;
        r->plan.valid = false;      // voices are matched differently
        r->matcher.reset();
    });
}

namespace {
fr_status fill_dense(fr_renderer *r, float *out, uint32_t n_slots, uint64_t n_times, uint64_t idx, const float *in, uint32_t n_in_rows,
                     bool device, void *stream) {
    if (!r) return FR_ERR_INVALID_ARG;
    if (n_in_rows && n_times && !in) { r->last_error = "null input matrix"; return FR_ERR_INVALID_ARG; }
    const uint32_t stored = std::min(n_in_rows, r->track_from);
    std::vector<uint64_t> offs((size_t)stored + 1);
    for (uint32_t i = 0; i <= stored; ++i) offs[i] = (uint64_t)i * n_times;
    r->dense_total_rows = n_in_rows;
    const fr_status st = device ? fr_fill_buffer_device(r, out, n_slots, n_times, idx, in, offs.data(), stored, stream)
                                : fr_fill_buffer(r, out, n_slots, n_times, idx, in, offs.data(), stored);
    r->dense_total_rows = 0;
    return st;
}
}   // namespace

fr_status fr_fill_buffer_dense(fr_renderer *r, float *out, uint32_t n_slots, uint64_t n_times, uint64_t idx, const float *in, uint32_t n_in_rows) {
    return fill_dense(r, out, n_slots, n_times, idx, in, n_in_rows, false, nullptr);
}
fr_status fr_fill_buffer_device_dense(fr_renderer *r, float *d_out, uint32_t n_slots, uint64_t n_times, uint64_t idx, const float *d_in,
                                      uint32_t n_in_rows, void *stream) {
    return fill_dense(r, d_out, n_slots, n_times, idx, d_in, n_in_rows, true, stream);
}

fr_status fr_host_register(fr_renderer *r, void *p, size_t bytes) {
    return guarded(r, [&] {
        if (!p || !bytes) throw Error(FR_ERR_INVALID_ARG, "empty range");
        HIP_CHECK(hipSetDevice(r->device));
        HIP_CHECK(hipHostRegister(p, bytes, hipHostRegisterMapped));
        r->registered.push_back({(char *)p, bytes});
    });
}

fr_status fr_host_unregister(fr_renderer *r, void *p) {
    return guarded(r, [&] {
        HIP_CHECK(hipSetDevice(r->device));
        for (size_t i = 0; i < r->registered.size(); ++i)
            if (r->registered[i].first == (char *)p) { r->registered.erase(r->registered.begin() + (ptrdiff_t)i); break; }
        HIP_CHECK(hipHostUnregister(p));
    });
}

fr_status fr_comm_unique_id(uint8_t id[FR_COMM_ID_BYTES]) {
    if (!id) return FR_ERR_INVALID_ARG;
    try {
        rccl_unique_id(id);
        return FR_OK;
    } catch (const Error &e) {
        return e.code;
    }
}

// ---- block streaming ------------------------------------------------------------------------------------------------------
fr_status fr_stream_begin(fr_renderer *r, uint32_t n_slots) {
    return guarded(r, [&] {
        HIP_CHECK(hipSetDevice(r->device));
        if (n_slots == 0) throw Error(FR_ERR_INVALID_ARG, "no output slots");
        if (r->sharded()) throw Error(FR_ERR_UNSUPPORTED, "block streaming of a sharded renderer");
        r->order_after_previous(r->stream);
        r->ensure_plan(n_slots, r->stream);
        const StagedPlan &sp = r->plan.sp;
        if (stream_path(sp, r->stream_bank_list(), r->stream_env())) {
            r->begin_program_stream(n_slots);
            return;
        }
        // what one resident launch can serve: every row straight from one balanced template voice, nothing stored between calls
        if (!r->plan_is_stateless(n_slots) || r->plan.banks.size() != 1)
            throw Error(FR_ERR_UNSUPPORTED, "block streaming needs a plan that is one voice bank (this one: " + std::to_string(r->plan.banks.size()) + " bank launches, " +
                                                std::to_string(sp.progs.size()) + " programs, " + std::to_string(r->plan.pull_rows.size()) + " pull rows" +
                                                (sp.uses_rings() ? ", rings" : "") + (r->plan_current(n_slots) ? "" : ", plan not current") + ")");
        const BankStage &bs = r->plan.banks[0];
        if (bs.grp.general || bs.grp.jit || bs.grp.to_ring || bs.grp.to_ws || bs.grp.rows.size() != n_slots || !sp.pull_rows.empty())
            throw Error(FR_ERR_UNSUPPORTED, "block streaming needs balanced template voices, one per output row");
        if (r->bank_tune.leaf_variant != 1) throw Error(FR_ERR_UNSUPPORTED, "block streaming with FR_BANK_LEAF=0");
        if (bs.grp.input_slot != 0) throw Error(FR_ERR_UNSUPPORTED, "block streaming feeds input slot 0; these voices read another slot");
        if (bs.grp.log2_p < 7) throw Error(FR_ERR_UNSUPPORTED, "block streaming needs voices of at least 128 partials (16 waves x one group of 8)");
        // Every workgroup of the launch must be resident at once (a workgroup that never starts never counts its voice in), one
        // per CU: as many as the device has CUs (a partitioned gfx950 has fewer than 256), and no more than the kernel's limit.
        const uint64_t max_wgs = std::min<uint64_t>(BANK_STREAM_WGS, (uint64_t)std::max(r->device_cus, 1));
        fr_renderer::Stream::Open o;
        StreamBank sb;
        if (!plain_stream_launch(n_slots, bs.grp.log2_p, max_wgs, sb, o.launch))
            throw Error(FR_ERR_UNSUPPORTED, "block streaming serves at most one voice per CU (" + std::to_string(max_wgs) + " here)");
        r->ensure_stream_buffers(o.launch, n_slots);
        StreamLaunchArgs x{};
        x.a = r->stream_bank_args(&bs, n_slots, sb.chunk_log2, 1u << (sb.log2_p - sb.chunk_log2));
        r->launch_resident(o, x);
        r->open_stream(std::move(o), n_slots);
    });
}

// One block of the open stream: `n_rows` input rows in fr_fill_buffer's shape (row i feeds input slot i).  Statuses and output
// bits are fr_fill_buffer's for the same sequence of calls: the input store's rules are kept for the rows without storing them
// (streamrows.hpp), and the rows of the slots the plan reads (StreamPlan::input_slots; a plan without FR_STREAM_INPUTS: slot 0)
// are the doorbell.
// `dense`, `dense_rows`: the block came as an [dense_rows][n_times] matrix (fr_stream_block_dense; the rows above are its rows
// below the first track slot); a stream of track voices (FR_STREAM_TRACKS) stages its rows from the first track slot on.
static void stream_block_rows(fr_renderer *r, float *out, uint64_t n_times, uint64_t idx, const float *in_data, const uint64_t *offs, uint32_t n_rows,
                              const float *dense = nullptr, uint32_t dense_rows = 0) {
    if (n_rows && !offs) throw Error(FR_ERR_INVALID_ARG, "null row offsets");
    if (n_rows && offs[n_rows] > offs[0] && !in_data) throw Error(FR_ERR_INVALID_ARG, "null input data");
    if (r->track_from != 0xFFFFFFFFu && n_rows > r->track_from) throw Error(FR_ERR_UNSUPPORTED, "block streaming takes no rows of track slots");
    // the first block of a stream, and a block that does not continue the previous one, is a seek: every slot unfed, every
    // input before idx 0.0.  A refused block changes nothing: the next one may follow as if it had not been made.
    fr_renderer::Stream::Open &o = r->strm.now;
    // (a stream that stores its rows, FR_STREAM_STORE: a block is a seek when it does not continue the RENDERER's head, which every
    //  answered block moves; the first block of a stream that does continue finds the rows' books in the store)
    const bool seek = o.store ? idx != r->head : !o.have_last || idx != o.head || (o.prog && !o.launched);
    if (o.store && !seek && !o.rows_open) {
        stream_rows_from_store(o.rows, r->n_vecs, r->segs, r->slots, r->last_stored_values());
        o.rows_open = true;
    }
    {
        std::string why;
        const StreamRowsStatus rs = o.rows.check(o.slots, n_times, idx, seek, offs, n_rows, &why);
        if (rs != STREAM_ROWS_OK) throw Error(rs == STREAM_ROWS_HISTORY ? FR_ERR_INPUT_HISTORY : FR_ERR_INPUT_TOO_LONG, why);
    }
    // a plan with programs: the rings are brought up to idx and the resident launch starts there
    const uint32_t rows_fed = o.store ? store_rows_taken(o.rows.n_vecs, o.slots, n_times, n_rows) : 0;
    if (o.store) {
        // append in place, or (re)launch first: a seek, the stream's first block, a slot more, no room in a slot's buffer
        if (seek || !o.launched || stream_store_block_relaunches(o.streamed, r->slots, rows_fed, r->keep_frames(), idx, n_times)) {
            const bool first = !o.have_last && !o.launched;
            r->launch_store_stream(idx, rows_fed, seek);
            if (first) o.continued = !seek;
        } else {
            r->history_floor = store_floor(r->history_floor, r->keep_frames(), idx);
        }
    } else if (o.prog && seek) r->seek_program_stream(idx);
    const auto t_in = std::chrono::steady_clock::now();
    // the rows of the slots the plan reads, padded like short rows of fill_buffer (reference.rs:72-73); a slot without a row: +0.0
    // (a one-row doorbell: StreamPlan::input_slots is {0}, also in a stream of the plain path, which has no plan)
    const uint32_t K = o.launch.n_rows;
    float rows[BANK_STREAM_ROWS][STREAM_ROW_FRAMES];
    uint32_t want[BANK_STREAM_ROWS] = {0};
    if (o.store)
        for (uint32_t j = 0; j < K && j < o.streamed.size(); ++j) want[j] = o.streamed[j].slot;
    o.rows.accept(o.slots, n_times, idx, seek, in_data, offs, n_rows, o.store ? want : o.plan.input_slots.data(), K, rows);
    o.rows_open = true;
    if (!o.store) r->n_vecs = std::max(r->n_vecs, o.rows.n_vecs);   // (the count the stream reached stays with the renderer)
    if (o.prog && o.plan.has_tracks()) {
        // the block's tracks (kernels.hpp StreamTrackArgs): the slot limit is the dense call's (store_inputs: rows at or beyond the
        // vector count are dropped; no matrix, or none that reaches the first track slot: every track reads +0.0), the rows from the
        // first track slot below it go to the staging, stride 64, then the control word, all before the doorbell's words.  One
        // buffer: the previous block's done tag followed every workgroup's last track read.
        const uint32_t from = o.plan.track_first;
        const uint64_t have = dense ? std::min<uint64_t>(dense_rows, o.rows.n_vecs) : 0;
        const uint32_t limit = have > from ? (uint32_t)have : 0u;
        const uint32_t staged = limit ? std::min(limit - from, o.plan.track_rows) : 0u;
        if (from != r->track_from || (size_t)o.plan.track_rows * STREAM_BLOCK * sizeof(float) > r->strm.h_trk.bytes || !o.launch.rows_doorbell)
            throw Error(FR_ERR_DEVICE, "internal: the track staging is not the plan's");
        float *stage = r->strm.h_trk.as<float>();
        const float *first = staged ? dense + (uint64_t)from * n_times : nullptr;
        if (staged && n_times == STREAM_BLOCK) std::memcpy(stage, first, (size_t)staged * STREAM_BLOCK * sizeof(float));
        else for (uint32_t q = 0; q < staged; ++q) std::memcpy(stage + (size_t)q * STREAM_BLOCK, first + (uint64_t)q * n_times, n_times * sizeof(float));
        __atomic_thread_fence(__ATOMIC_RELEASE);
        __atomic_store_n(&static_cast<BankStreamInCtl *>(r->strm.h_ctl.p)->tracks, (unsigned long long)staged << 32 | limit, __ATOMIC_RELAXED);
        __atomic_thread_fence(__ATOMIC_RELEASE);
    }
    // every word is tagged with the block's number and length: the words are the doorbell (kernels.hpp BankStreamCtl, BankStreamInCtl)
    o.seq = (o.seq + 1u) & 0xFFFFFFu;
    if (o.seq == 0 || o.seq == 0xFFFFFFu) o.seq = 1;
    const uint32_t seq = o.seq << 8 | (uint32_t)n_times;
    const StreamDoorbell bell = stream_doorbell(r->strm.h_ctl.p, o.launch.rows_doorbell);
    for (uint32_t j = 0; j < K; ++j)
        for (uint64_t i = 0; i < 64; ++i) {
            uint32_t bits;
            std::memcpy(&bits, &rows[j][i], 4);
            __atomic_store_n(&bell.words[(size_t)j * 64 + i], (unsigned long long)seq << 32 | bits, __ATOMIC_RELAXED);
        }
    uint64_t spins = 0;
    const auto t_ring = std::chrono::steady_clock::now();
    while (__atomic_load_n(bell.done, __ATOMIC_ACQUIRE) != seq) {
        if ((++spins & 0xFFFFFu) != 0) continue;
        if (hipStreamQuery(r->stream) != hipErrorNotReady) {   // the launch is gone (its own bound, or a fault)
            (void)hipStreamSynchronize(r->stream);
            o.launched = false;
            r->end_stream(false);                              // (it may have ended between two chunks of a voice)
            throw Error(FR_ERR_DEVICE, "the resident launch ended before the block was rendered");
        }
        // a resident launch answers in tens of microseconds; a quarter of a second without an answer means it is not all
        // resident (something else holds CUs) or the device is in trouble: give the audio thread back
        if (std::chrono::steady_clock::now() - t_ring > std::chrono::milliseconds(250)) {
            r->end_stream(false);
            throw Error(FR_ERR_DEVICE, "the resident launch did not answer within 250 ms");
        }
    }
    const auto t_done = std::chrono::steady_clock::now();
    const float *res = r->strm.h_out.as<float>();
    for (uint32_t v = 0; v < o.slots; ++v) std::memcpy(out + (size_t)v * n_times, res + (size_t)v * 64, n_times * sizeof(float));
    o.head = idx + n_times;
    o.have_last = true;
    if (o.store) r->commit_streamed_block(rows_fed, idx, n_times);   // (a done tag implies the block's rows are in the store)
    if (r->host_trace) {   // FR_HOST_TRACE=1: inside the call, without the caller's wrapper
        r->strm.trace_us[0] += std::chrono::duration<double, std::micro>(t_done - t_in).count();
        r->strm.trace_us[1] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_done).count();
        ++r->strm.trace_n;
    }
}

fr_status fr_stream_block_rows(fr_renderer *r, float *out, uint64_t n_times, uint64_t idx, const float *in_data, const uint64_t *in_row_offsets, uint32_t n_in_rows) {
    return guarded(r, [&] {
        if (!r->strm.open) throw Error(FR_ERR_INVALID_ARG, "no stream is open (fr_stream_begin; any other call on the renderer closes it)");
        if (!out || n_times == 0 || n_times > 64) throw Error(FR_ERR_INVALID_ARG, "a streamed block is 1..64 frames");
        stream_block_rows(r, out, n_times, idx, in_data, in_row_offsets, n_in_rows);
    }, true);
}

// (one row, for input slot 0: fr_stream_block_rows with that row)
fr_status fr_stream_block(fr_renderer *r, float *out, uint64_t n_times, uint64_t idx, const float *row, uint64_t row_len) {
    return guarded(r, [&] {
        if (!r->strm.open) throw Error(FR_ERR_INVALID_ARG, "no stream is open (fr_stream_begin; any other call on the renderer closes it)");
        if (!out || n_times == 0 || n_times > 64 || row_len > n_times || (row_len && !row)) throw Error(FR_ERR_INVALID_ARG, "a streamed block is 1..64 frames");
        const uint64_t offs[2] = {0, row_len};
        stream_block_rows(r, out, n_times, idx, row, offs, 1);
    }, true);
}

// (the block as a dense matrix: its rows below the first track slot are fr_stream_block_rows' rows, full length; the rows from
// that slot on are the block's tracks)
fr_status fr_stream_block_dense(fr_renderer *r, float *out, uint64_t n_times, uint64_t idx, const float *in, uint32_t n_in_rows) {
    return guarded(r, [&] {
        if (!r->strm.open) throw Error(FR_ERR_INVALID_ARG, "no stream is open (fr_stream_begin; any other call on the renderer closes it)");
        if (!out || n_times == 0 || n_times > 64) throw Error(FR_ERR_INVALID_ARG, "a streamed block is 1..64 frames");
        if (n_in_rows && !in) throw Error(FR_ERR_INVALID_ARG, "null input matrix");
        const uint32_t stored = std::min(n_in_rows, r->track_from);
        std::vector<uint64_t> offs((size_t)stored + 1);
        for (uint32_t i = 0; i <= stored; ++i) offs[i] = (uint64_t)i * n_times;
        stream_block_rows(r, out, n_times, idx, in, offs.data(), stored, in, n_in_rows);
    }, true);
}

fr_status fr_stream_end(fr_renderer *r) {
    return guarded(r, [&] { HIP_CHECK(hipSetDevice(r->device)); });   // (guarded() itself retires the launch)
}

fr_status fr_comm_selftest(int32_t device, uint64_t n_floats) {
    if (n_floats == 0 || n_floats > (1ull << 26)) return FR_ERR_INVALID_ARG;   // (256 MB each way is plenty for a check)
    float *d_send = nullptr, *d_recv = nullptr;
    hipStream_t st = nullptr;
    fr_status rc = FR_OK;
    try {
        if (device >= 0) HIP_CHECK(hipSetDevice(device));
        uint8_t id[FR_COMM_ID_BYTES];
        rccl_unique_id(id);
        std::unique_ptr<Transport> t = make_rccl_transport(id, 0, 1);
        HIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        HIP_CHECK(hipMalloc((void **)&d_send, n_floats * sizeof(float)));
        HIP_CHECK(hipMalloc((void **)&d_recv, n_floats * sizeof(float)));
        std::vector<float> h(n_floats), back(n_floats, -1.0f);
        for (uint64_t i = 0; i < n_floats; ++i) h[i] = (float)(i % 8191) * 0.25f - 3.0f;
        HIP_CHECK(hipMemcpyAsync(d_send, h.data(), n_floats * sizeof(float), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(d_recv, 0xFF, n_floats * sizeof(float), st));
        t->sendrecv(0, d_send, n_floats, d_recv, n_floats, st);
        HIP_CHECK(hipMemcpyAsync(back.data(), d_recv, n_floats * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (std::memcmp(h.data(), back.data(), n_floats * sizeof(float)) != 0) rc = FR_ERR_COMM;
    } catch (const Error &e) {
        rc = e.code;
    } catch (...) {
        rc = FR_ERR_DEVICE;
    }
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (d_send) (void)hipFree(d_send);
    if (d_recv) (void)hipFree(d_recv);
    return rc;
}

fr_status fr_set_shard(fr_renderer *r, const fr_shard *sh) {
    return guarded(r, [&] {
        HIP_CHECK(hipSetDevice(r->device));
        HIP_CHECK(hipDeviceSynchronize());   // nothing of the previous arrangement is still in flight
        r->last_pending = false;
        ShardSpec spec;
        uint32_t flags = 0;
        std::unique_ptr<Transport> transport;
        fr_comm comm{};
        bool has_comm = false;
        if (sh && sh->world > 1 && sh->mode != FR_SHARD_NONE) {
            if (sh->mode != FR_SHARD_VOICES && sh->mode != FR_SHARD_PARTIALS) throw Error(FR_ERR_INVALID_ARG, "unknown shard mode");
            if (sh->world > 64 || sh->rank >= sh->world) throw Error(FR_ERR_INVALID_ARG, "shard rank/world out of range (world <= 64)");
            if (sh->mode == FR_SHARD_PARTIALS && (sh->world & (sh->world - 1)) != 0)
                throw Error(FR_ERR_INVALID_ARG, "partial-block sharding needs a power-of-two world size");
            if (sh->flags & ~(FR_SHARD_GATHER | FR_SHARD_SERIAL_EXCHANGE)) throw Error(FR_ERR_INVALID_ARG, "unknown shard flags");
            spec.rank = sh->rank;
            spec.world = sh->world;
            spec.mode = sh->mode;
            flags = sh->flags;
            if (sh->comm) {
                if (!sh->comm->sendrecv) throw Error(FR_ERR_INVALID_ARG, "fr_comm without a sendrecv function");
                comm = *sh->comm;
                has_comm = true;
            }
            if (sh->rccl_id) transport = make_rccl_transport(sh->rccl_id, sh->rank, sh->world);   // collective
        }
        // Partial-block sharding needs every rank to arrive at the SAME plan (the same list of split voices) on the same
        // call; a kernel that finishes compiling at different moments on different ranks would break that, so compile in
        // the call from here on.
        // (and back to the configured behaviour when the renderer leaves that mode)
        r->jit_cache.set_async(spec.mode == FR_SHARD_PARTIALS ? false : r->jit_async_configured);
        r->shard = spec;
        r->shard_flags = flags;
        r->rccl = std::move(transport);
        r->host_comm = comm;
        r->has_host_comm = has_comm;
        ++r->shard_epoch;                    // the plan depends on all of it
    });
}

fr_status fr_shard_rows(const fr_renderer *r, uint32_t n_slots, uint32_t *lo, uint32_t *hi) {
    if (!r || !lo || !hi) return FR_ERR_INVALID_ARG;
    r->my_rows(n_slots, *lo, *hi);
    return FR_OK;
}

const char *fr_last_error(const fr_renderer *r) { return r ? r->last_error.c_str() : "null renderer"; }

const char *fr_status_string(fr_status s) {
    switch (s) {
    case FR_OK: return "ok";
    case FR_ERR_INVALID_ARG: return "invalid argument";
    case FR_ERR_INPUT_TOO_LONG: return "input row extends past the rendered range";
    case FR_ERR_INPUT_HISTORY: return "input row does not continue the slot's stored history";
    case FR_ERR_NO_SUCH_NODE: return "no such node";
    case FR_ERR_BAD_SLOT: return "primitive read through a non-zero output slot";
    case FR_ERR_CYCLE: return "dependency cycle";
    case FR_ERR_DEVICE: return "device error";
    case FR_ERR_NO_DEVICE: return "no usable gfx950 device";
    case FR_ERR_OUT_OF_MEMORY: return "out of memory";
    case FR_ERR_UNSUPPORTED: return "unsupported";
    case FR_ERR_COMM: return "communication error";
    default: return "unknown status";
    }
}

const char *fr_backend_name(void) { return "hip-gfx950"; }
uint32_t fr_abi_version(void) { return FR_ABI_VERSION; }

const char *fr_plan_json(fr_renderer *r) {
    if (!r) return "{}";
    r->plan_json_cache = r->plan.valid ? r->plan.json : "{}";
    if (r->plan.valid && r->plan_json_cache.size() > 1) {   // live: counters of the exchange step (partial-block sharding), the last call's bank launches
        r->plan_json_cache.pop_back();
        r->plan_json_cache += ",\"lookback_growths\":" + std::to_string(r->lookback_growths) + ",\"range_launches\":" + std::to_string(r->range_launches);
        r->plan_json_cache += ",\"track_tail_bytes\":" + std::to_string((uint64_t)r->tail_rows * r->tail_cap * sizeof(float)) +
                              ",\"track_tail_launches\":" + std::to_string(r->tail_launches);
        if (r->ring_keep) {
            const fr_renderer::RingState &rs = r->ring_state;
            r->plan_json_cache += ",\"ring_state\":{\"kept\":" + std::to_string(rs.kept) + ",\"rebuilt\":" + std::to_string(rs.rebuilt) +
                                  ",\"moved\":" + std::to_string(rs.moved) + ",\"move_launches\":" + std::to_string(rs.move_launches) +
                                  ",\"repair_from\":" + std::to_string(rs.repair_from) + ",\"inert\":\"" + rs.inert + "\"}";
        }
        if (r->stream_programs) {
            const StreamPlan s = r->plan_stream_now();
            std::string per;
            for (uint32_t n : s.programs_per_voice()) per += (per.empty() ? "" : ",") + std::to_string(n);
            std::string ins;
            for (uint32_t n : s.input_slots) ins += (ins.empty() ? "" : ",") + std::to_string(n);
            std::string why;
            for (char c : s.reason) { if (c == '"' || c == '\\') why += '\\'; why += c; }
            r->plan_json_cache += std::string(",\"stream\":{\"servable\":") + (s.servable ? "true" : "false") + ",\"reason\":\"" + why +
                                  "\",\"voices\":" + std::to_string(s.voices) + ",\"chunks\":" + std::to_string(s.chunks) + ",\"programs_per_voice\":[" + per +
                                  "],\"bus_programs\":" + std::to_string(s.bus_programs()) + ",\"min_ring_delay\":" + std::to_string(s.min_ring_delay) + ",\"rings\":" + std::to_string(r->plan.sp.n_rings) +
                                  ",\"input_slots\":[" + ins + "]";
            if (r->stream_loops) {                               // FR_STREAM_LOOPS: the stride of each streamed program, in the order they run
                std::string lp;
                for (uint32_t l : s.loop_stride) lp += (lp.empty() ? "" : ",") + std::to_string(l);
                r->plan_json_cache += ",\"loop_programs\":[" + lp + "],\"loop_loads\":" + std::to_string(STREAM_LOOP_LOADS) + ",\"loop_stores\":" + std::to_string(STREAM_LOOP_STORES);
            }
            // (the kernel a servable plan will get where the plan decides it; else the last resident launch's, unless that was one of those)
            if (r->stream_general) {                             // FR_STREAM_GENERAL: the leaves of every voice served by schedule, by global voice
                std::string gv;
                for (uint32_t n : s.general_voices) gv += (gv.empty() ? "" : ",") + std::to_string(n);
                r->plan_json_cache += ",\"general_voices\":[" + gv + "],\"general_max_leaves\":" + std::to_string(STREAM_GENERAL_MAX_LEAVES);
            }
            if (r->stream_dyn)                                   // FR_STREAM_DYN: the assigned programs' Delays by a signal amount, and the deepest ring read
                r->plan_json_cache += ",\"dyn_reads\":" + std::to_string(s.dyn_reads) + ",\"dyn_steps\":" + std::to_string(s.dyn_steps) +
                                      ",\"lookback\":" + std::to_string(s.lookback);
            if (r->stream_history)                               // FR_STREAM_HISTORY: the assigned programs' delayed reads of input rows, and the deepest of them
                r->plan_json_cache += ",\"hist_reads\":" + std::to_string(s.hist_reads) + ",\"hist_dyn_reads\":" + std::to_string(s.hist_dyn_reads) +
                                      ",\"input_lookback\":" + std::to_string(s.input_lookback);
            if (r->stream_effects)                               // FR_STREAM_EFFECTS: the workgroups a plan without a voice is dealt over (0: it has voices)
                r->plan_json_cache += ",\"segments\":" + std::to_string(s.segments);
            if (r->stream_taps)                                  // FR_STREAM_TAPS: the levels of the run form, the reads below a block of rings that programs store
                r->plan_json_cache += ",\"levels\":" + std::to_string(s.levels) + ",\"short_reads\":" + std::to_string(s.short_reads) +
                                      ",\"dyn_ring_reads\":" + std::to_string(s.dyn_ring_reads);
            if (r->stream_leaves) {                              // FR_STREAM_LEAVES: the leaf banks' programs, in plan order ([]: the plan has none)
                std::string lb;
                for (size_t i = 0; i < s.leaf_progs.size() && i < s.banks.size(); ++i)
                    if (s.banks[i].leaf)
                        lb += std::string(lb.empty() ? "" : ",") + "{\"ops\":" + std::to_string(s.leaf_progs[i].ins.size()) + ",\"regs\":" + std::to_string(s.leaf_progs[i].regs) +
                              ",\"params\":" + std::to_string(s.leaf_progs[i].k) + ",\"inputs\":" + std::to_string(s.leaf_progs[i].inputs_read) +
                              (r->stream_tracks ? ",\"track_cols\":" + std::to_string(s.leaf_progs[i].track_cols.size()) : std::string()) + "}";
                r->plan_json_cache += ",\"leaf_banks\":[" + lb + "]";
            }
            if (r->stream_tracks)                                // FR_STREAM_TRACKS: the staged rows (0: no leaf reads a track) and their limit
                r->plan_json_cache += ",\"tracks\":{\"first_slot\":" + std::to_string(s.has_tracks() ? s.track_first : 0) + ",\"rows\":" + std::to_string(s.track_rows) +
                                      ",\"limit\":" + std::to_string(STREAM_MAX_TRACK_ROWS) + "}";
            if (r->stream_sweep) {                               // FR_STREAM_SWEEP: the width of every streamed program, in the order of `progs` (0: no sweep program)
                std::string sw;
                for (uint32_t w : s.sweep_width) sw += (sw.empty() ? "" : ",") + std::to_string(w);
                r->plan_json_cache += ",\"sweep_programs\":[" + sw + "]";
            }
            const StreamLaunch l = s.servable ? stream_launch(r->plan.sp, s) : StreamLaunch{};
            const char *kernel = stream_kernel_name(l.by_plan ? l.kernel : stream_kernel_by_plan(r->strm.last_kernel) ? StreamKernel::none : r->strm.last_kernel);
            if (r->stream_banks) {                               // FR_STREAM_BANKS: the banks of the launch, in plan order
                std::string bl;
                for (const StreamBank &b : s.banks)
                    bl += std::string(bl.empty() ? "" : ",") + "{\"voices\":" + std::to_string(b.voices) + ",\"partials\":" + std::to_string(b.general ? b.max_leaves : 1u << b.log2_p) +
                          ",\"chunks\":" + std::to_string(1u << (b.log2_p - b.chunk_log2)) + ",\"to_ring\":" + (b.to_ring ? "true" : "false") +
                          (r->stream_general ? std::string(",\"general\":") + (b.general ? "true" : "false") : std::string()) + "}";
                r->plan_json_cache += ",\"banks\":[" + bl + "],\"workgroups\":" + std::to_string(s.servable && s.voices == 0 ? s.segments : s.workgroups()) +   // (without a voice: the segments)
                                      ",\"max_workgroups\":" + std::to_string(stream_max_wgs((uint32_t)std::max(r->device_cus, 0)));
            }
            if (r->stream_store) {                               // FR_STREAM_STORE: whether it acts, the slots such a stream streams, the open stream's first block and relaunches
                const std::string inert = r->stream_store_inert_now();
                const fr_renderer::Stream::Open &o = r->strm.now;
                std::vector<uint32_t> ss;
                if (r->strm.open && o.store && !o.streamed.empty())
                    for (const StoreStreamed &x : o.streamed) ss.push_back(x.slot);
                else if (inert.empty()) (void)stream_store_slots(s.input_slots, r->slots, 0, ss);
                std::string sl;
                for (uint32_t n : ss) sl += (sl.empty() ? "" : ",") + std::to_string(n);
                r->plan_json_cache += std::string(",\"store\":{\"on\":") + (inert.empty() ? "true" : "false") + ",\"slots\":[" + sl + "],\"continued\":" +
                                      (r->strm.open && o.continued ? "true" : "false") + ",\"relaunches\":" + std::to_string(r->strm.open ? o.relaunches : 0u) +
                                      ",\"inert\":\"" + inert + "\"}";
            }
            r->plan_json_cache += std::string(",\"kernel\":\"") + kernel + "\"}";
        }
        r->plan_json_cache += ",\"exchange_stats\":{\"calls\":" + std::to_string(r->exchange_calls) + ",\"tiles\":" + std::to_string(r->exchange_tiles) +
                              ",\"bytes_sent\":" + std::to_string(r->exchange_bytes) + "},\"bank_launches\":[";
        for (size_t i = 0; i < r->bank_launches.size(); ++i) {
            const BankLaunchNote &b = r->bank_launches[i];
            r->plan_json_cache += std::string(i ? "," : "") + "{\"kernel\":\"" + b.launch.kernel + "\",\"voices\":" + std::to_string(b.voices) +
                                  ",\"partials\":" + std::to_string(b.partials) + ",\"frames\":" + std::to_string(b.frames) +
                                  ",\"chunk_log2\":" + std::to_string(b.launch.chunk_log2) + ",\"waves_per_group\":" + std::to_string(b.launch.waves_per_group) +
                                  ",\"frames_per_lane\":" + std::to_string(b.launch.frames_per_lane) + ",\"voices_per_wave\":" + std::to_string(b.launch.voices_per_wave) +
                                  ",\"publishes_rows\":" + (b.launch.publishes_rows ? "true" : "false") + ",\"leaf_variant\":" + std::to_string(b.leaf_variant) +
                                  ",\"small_call\":" + std::to_string(b.launch.small_call) + ",\"pieces_log2\":" + std::to_string(b.launch.pieces_log2) +
                                  ",\"variant\":\"" + bank_variant(b.launch, b.log2_p, b.leaf_variant, b.row_flags) + "\"" +
                                  (r->ring_keep ? std::string(",\"form\":\"") + b.form + "\"" : std::string()) + "}";
        }
        r->plan_json_cache += "],\"stage_launches\":[";
        for (size_t i = 0; i < r->stage_launches.size(); ++i) {
            const StageLaunchNote &n = r->stage_launches[i];
            r->plan_json_cache += std::string(i ? "," : "") + "{\"form\":\"" + n.form + "\",\"kernel\":\"" + (n.jit ? "jit_stage" : "stage_kernel") +
                                  "\",\"programs\":" + std::to_string(n.programs) + ",\"frames\":" + std::to_string(n.frames) +
                                  ",\"stride\":" + std::to_string(n.stride) + ",\"carry\":" + (n.carry ? "true" : "false") +
                                  ",\"carry_only\":" + (n.carry_only ? "true" : "false") + ",\"table_inputs\":" + (n.table ? "true" : "false") +
                                  ",\"grid_parts\":" + std::to_string(n.grid_parts) + ",\"variant\":\"" + stage_variant(n, r->plan) + "\"}";
        }
        r->plan_json_cache += "]}";
    }
    return r->plan_json_cache.c_str();
}

const char *fr_options_json(fr_renderer *r) {
    if (!r) return "{}";
    static const char *const kSource[] = {"default", "env", "option"};
    std::string &js = r->options_json_cache;
    js = "{";
    for (size_t i = 0; i < N_OPTIONS; ++i)
        if (kKnobs[i].listed == LISTED || (kKnobs[i].listed == LISTED_WHEN_SET && r->option_source[i] != OPTION_DEFAULT))
            js += std::string(js.size() > 1 ? "," : "") + "\"" + kKnobs[i].name + "\":{\"value\":\"" + option_text(kKnobs[i], r->option_value[i]) +
              "\",\"source\":\"" + kSource[r->option_source[i]] + "\"}";
    js += "}";
    return js.c_str();
}

fr_status fr_set_timing(fr_renderer *r, int32_t enabled) {
    if (!r) return FR_ERR_INVALID_ARG;
    r->timing = enabled != 0;
    return FR_OK;
}

fr_status fr_get_timing(fr_renderer *r, const char *kernel_class, double *ms, uint64_t *launches) {
    return guarded(r, [&] {
        if (!kernel_class) throw Error(FR_ERR_INVALID_ARG, "null kernel class");
        HIP_CHECK(hipSetDevice(r->device));
        r->resolve(r->t_bank);
        r->resolve(r->t_pull);
        r->resolve(r->t_stage);
        std::string k(kernel_class);
        double m = 0;
        uint64_t n = 0;
        if (k == "bank" || k == "all") { m += r->t_bank.ms; n += r->t_bank.launches; }
        if (k == "pull" || k == "all") { m += r->t_pull.ms; n += r->t_pull.launches; }
        if (k == "stage" || k == "all") { m += r->t_stage.ms; n += r->t_stage.launches; }
        if (k != "bank" && k != "pull" && k != "all" && k != "stage") throw Error(FR_ERR_INVALID_ARG, "unknown kernel class " + k);
        if (ms) *ms = m;
        if (launches) *launches = n;
    });
}

fr_status fr_reset_timing(fr_renderer *r) {
    return guarded(r, [&] {
        HIP_CHECK(hipSetDevice(r->device));
        r->resolve(r->t_bank);
        r->resolve(r->t_pull);
        r->resolve(r->t_stage);
        r->t_bank.ms = r->t_pull.ms = r->t_stage.ms = 0;
        r->t_bank.launches = r->t_pull.launches = r->t_stage.launches = 0;
    });
}

}  // extern "C"
