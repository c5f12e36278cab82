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
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "stage.hpp"

namespace fr {

constexpr uint32_t STREAM_BLOCK = 64;        // the longest block a stream accepts
constexpr uint32_t STREAM_MAX_WGS = 256;     // (= kernels.hpp BANK_STREAM_WGS)
constexpr uint32_t STREAM_MAX_INPUTS = 8;    // most distinct input slots the streamed programs may read, slot 0 included (= kernels.hpp BANK_STREAM_ROWS)
constexpr uint32_t STREAM_MAX_BANKS = 8;     // most bank launches one resident launch serves (= kernels.hpp BANK_STREAM_BANKS)

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
};

// One bank of a streamed plan.  Voices [first_voice, first_voice + voices) of the global numbering; workgroups
// [first_wg, first_wg + (voices << (log2_p - chunk_log2))) of the launch, voice-major, then chunk.
struct StreamBank {
    uint32_t first_voice = 0, voices = 0, log2_p = 0, chunk_log2 = 0;
    bool to_ring = false;
    uint32_t first_wg = 0;
};

// Every workgroup of the launch must be resident at once, one per CU: as many as the device has CUs (0: unknown, the kernel's
// own limit stands in), and no more than the kernel's limit.
inline uint64_t stream_max_wgs(uint32_t device_cus) { return std::min<uint64_t>(STREAM_MAX_WGS, device_cus ? device_cus : STREAM_MAX_WGS); }

// The chunk size of every bank (voices, log2_p set; chunk_log2 and first_wg are written).  Every bank starts at one chunk per
// voice; false when even that is more than max_wgs workgroups.  Then, until no bank qualifies: the bank with the largest chunk
// (on a tie the lower index) among those whose chunk is above 128 partials (a wave needs a group of 8), that have fewer than
// 256 chunks per voice and whose halving keeps the total within max_wgs, has its chunk halved.  A block is only as fast as its
// largest chunk, so this evens out the partials per workgroup; for one bank it is the short-call kernel's loop.
inline bool deal_stream_chunks(std::vector<StreamBank> &banks, uint64_t max_wgs) {
    uint64_t total = 0;
    for (StreamBank &b : banks) { b.chunk_log2 = b.log2_p; total += b.voices; }
    if (total > max_wgs) return false;
    for (;;) {
        StreamBank *pick = nullptr;
        for (StreamBank &b : banks) {
            if (!(b.chunk_log2 > 7 && b.log2_p - b.chunk_log2 < 8)) continue;
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

struct StreamPlan {
    bool servable = false;
    std::string reason;              // why not ("" when servable)
    uint32_t voices = 0, chunk_log2 = 0, chunks = 0;   // chunks per voice; one bank: the launch has voices * chunks workgroups
    bool bank_to_ring = false;
    std::vector<StreamBank> banks;       // one per bank launch, in plan order.  Several: `voices` is their total, `chunks` the
                                         // largest per-voice chunk count, chunk_log2 / bank_to_ring are bank 0's
    uint32_t workgroups() const {
        uint32_t n = 0;
        for (const StreamBank &b : banks) n += b.voices << (b.log2_p - b.chunk_log2);
        return n;
    }
    std::vector<uint32_t> progs;         // indices into StagedPlan::progs, voice by voice, then the bus programs, in the order they run
    std::vector<uint32_t> voice_first;   // [voices + 2] into `progs`: [voice_first[voices], voice_first[voices + 1]) is the bus segment
    uint64_t min_ring_delay = 0;         // shortest delayed read of a ring that a program stores (0: there is none)
    uint64_t lookback = 0;               // deepest ring read of the assigned programs
    std::vector<uint32_t> input_slots{0};   // the distinct input slots the voices and the assigned programs read: slot 0 (the voices' time)
                                         // first, the others ascending -- the order of a block's streamed rows
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

// `banks`: the plan's bank launches (the engine moves them out of StagedPlan::banks when it uploads them).
inline StreamPlan plan_stream(const StagedPlan &sp, const std::vector<const BankLaunch *> &banks, const StreamEnv &env) {
    StreamPlan s;
    auto refuse = [&](const std::string &why) {
        s.servable = false;
        s.reason = why;
        if (!s.voices) s.banks.clear();              // (refused before the banks were dealt)
        return s;
    };
    if (env.n_slots == 0) return refuse("no output slots");
    if (env.sharded || !sp.split.empty()) return refuse("block streaming of a sharded renderer");
    if (env.pull_mode) return refuse("block streaming of a renderer in FR_MODE_PULL");
    if (!sp.pull_rows.empty()) return refuse(std::to_string(sp.pull_rows.size()) + " output rows are left to the pull interpreter");
    if (env.track_history || !sp.track_window_slots.empty() || sp.track_lookback != 0) return refuse("block streaming with a track history");
    if (banks.size() != 1 && !(env.banks && banks.size() >= 2 && banks.size() <= STREAM_MAX_BANKS)) {
        if (env.banks && banks.size() > STREAM_MAX_BANKS)
            return refuse("block streaming serves at most " + std::to_string(STREAM_MAX_BANKS) + " voice banks in one launch (this plan: " +
                          std::to_string(banks.size()) + " bank launches)");
        return refuse("block streaming needs a plan with one voice bank (this one: " + std::to_string(banks.size()) + " bank launches)");
    }
    for (const BankLaunch *bp : banks) {             // (one bank: the checks and their order are what they have always been)
        const BankLaunch &b = *bp;
        if (b.general || b.jit || b.tracks || b.to_ws) return refuse("block streaming needs balanced template voices (these are general, compiled or track voices)");
        if (env.leaf_variant != 1) return refuse("block streaming with FR_BANK_LEAF=0");
        if (b.input_slot != 0) return refuse("block streaming feeds input slot 0; these voices read another slot");
        if (b.log2_p < 7) return refuse("block streaming needs voices of at least 128 partials (16 waves x one group of 8)");
        if (b.rows.empty()) return refuse("block streaming needs a plan with one voice bank (this one has no voices)");
        StreamBank sb;
        sb.voices = (uint32_t)b.rows.size();
        sb.log2_p = b.log2_p;
        sb.to_ring = b.to_ring;
        s.banks.push_back(sb);
    }
    // every workgroup of the launch must be resident at once, one per CU: chunks of >= 128 partials until the CUs are used
    const uint64_t max_wgs = stream_max_wgs(env.device_cus);
    if (!deal_stream_chunks(s.banks, max_wgs)) return refuse("block streaming serves at most one voice per CU (" + std::to_string(max_wgs) + " here)");
    uint32_t V = 0;
    for (const StreamBank &sb : s.banks) {
        V += sb.voices;
        s.chunks = std::max(s.chunks, 1u << (sb.log2_p - sb.chunk_log2));
    }
    s.voices = V;
    s.chunk_log2 = s.banks[0].chunk_log2;
    s.bank_to_ring = s.banks[0].to_ring;
    std::vector<uint32_t> others;                    // slots other than 0 that the assigned programs read (StreamEnv::inputs)

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
        if (levels != 1)
            return refuse("the plan has no fused form: a program's ring is read less than " + std::to_string(STREAM_BLOCK) +
                          " frames back (or the fused programs exceed the interpreter's budget)");
        for (uint32_t i = sp.level_first[only]; i < sp.level_first[only + 1]; ++i) run.push_back(i);
    }
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
    const uint32_t BUS = V;                                   // "voice" of a bus program: the segment after the last voice's
    std::vector<uint32_t> voice_of(run.size(), NONE);
    // FR_STREAM_BUS: a program is a bus program when, at a delay below a block, it reads the bank rings of two or more voices
    // or a ring that an earlier bus program stores (a feedback plan's row copy of such a ring included)
    auto is_bus = [&](uint32_t k) {
        if (!env.bus) return false;
        const StageProg &pg = sp.progs[run[k]];
        uint32_t one = NONE;
        for (uint32_t i = 0; i < pg.n_instr; ++i) {
            const StageInstr &in = sp.instrs[pg.first_instr + i];
            if (in.op != S_READ || in.d_lo >= STREAM_BLOCK) continue;
            auto bv = bank_ring_voice.find(in.buf);
            if (bv != bank_ring_voice.end()) {
                if (one != NONE && one != bv->second) return true;
                one = bv->second;
                continue;
            }
            auto st = stored_by.find(in.buf);
            if (st != stored_by.end() && st->second < k && voice_of[st->second] == BUS) return true;
        }
        return false;
    };
    uint64_t min_delay = UINT64_MAX;
    for (uint32_t k = 0; k < run.size(); ++k) {
        const StageProg &pg = sp.progs[run[k]];
        const bool copy = k >= first_copy;
        const bool bus = is_bus(k);
        uint32_t mine = NONE;
        for (uint32_t i = 0; i < pg.n_instr; ++i) {
            const StageInstr &in = sp.instrs[pg.first_instr + i];
            switch (in.op) {
            case S_CONST: case S_STEP: case S_SUM2: case S_MUL: case S_DIV: case S_MOD: case S_MIN: case S_STORE: break;
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
                if (bus && in.d_lo < STREAM_BLOCK) {                 // a ring an EARLIER program of the block stores: it has finished
                    auto st = stored_by.find(in.buf);
                    if (st != stored_by.end() && st->second < k) break;
                    return refuse("a program's ring is read " + std::to_string(in.d_lo) + " frames back; a streamed block needs delays of at least " +
                                  std::to_string(STREAM_BLOCK) + " frames");
                }
                if (copy && in.d_lo == 0) {                          // a row copy: after the program that stores the ring, on its voice
                    auto st = stored_by.find(in.buf);
                    if (st == stored_by.end() || voice_of[st->second] == NONE) return refuse("internal: a row copy of a ring no streamed program stores");
                    mine = voice_of[st->second];
                    break;
                }
                if (in.d_lo < STREAM_BLOCK)
                    return refuse("a program's ring is read " + std::to_string(in.d_lo) + " frames back; a streamed block needs delays of at least " +
                                  std::to_string(STREAM_BLOCK) + " frames");
                min_delay = std::min<uint64_t>(min_delay, in.d_lo);
                break;
            }
            default:
                return refuse(std::string("a program uses ") + stage_op_name(in.op) +
                              (in.op == S_READ_INPUT ? " (a delayed read of the input row)" : " (a Delay by a signal amount)") + ", which block streaming does not serve yet");
            }
            if (in.dst >= STAGE_REGS || in.a >= STAGE_REGS || in.b >= STAGE_REGS) return refuse("a program needs more registers than the streamed interpreter has");
        }
        if (pg.result_reg >= STAGE_REGS) return refuse("a program needs more registers than the streamed interpreter has");
        voice_of[k] = bus ? BUS : mine != NONE ? mine : run[k] % V;   // (reads no voice at a short delay: any one voice, the same every time)
    }
    std::sort(others.begin(), others.end());
    others.erase(std::unique(others.begin(), others.end()), others.end());
    if (1 + others.size() > STREAM_MAX_INPUTS)
        return refuse("the programs read " + std::to_string(1 + others.size()) + " distinct input slots (slot 0 included); block streaming feeds at most " +
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
    s.voice_first.assign(V + 2, 0);
    for (uint32_t k = 0; k < run.size(); ++k) ++s.voice_first[voice_of[k] + 1];
    for (uint32_t v = 0; v <= V; ++v) s.voice_first[v + 1] += s.voice_first[v];
    s.progs.resize(run.size());
    std::vector<uint32_t> at(s.voice_first.begin(), s.voice_first.end() - 1);
    for (uint32_t k = 0; k < run.size(); ++k) s.progs[at[voice_of[k]]++] = run[k];   // (stable: the order of `run` inside a voice)
    s.min_ring_delay = min_delay == UINT64_MAX ? 0 : min_delay;
    s.input_slots.insert(s.input_slots.end(), others.begin(), others.end());
    s.servable = true;
    return s;
}

}  // namespace fr
