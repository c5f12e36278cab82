// bankplan.hpp -- which oscillator-bank kernel a bank group's launch runs, and in what shape.  Plain host logic, no HIP
// runtime calls, all inline: the engine's launch, the input store's row deferral and the streamed host output ask the same
// rule, and the host-logic simulator compiles it with the engine.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>

#include "stage.hpp"

namespace fr {

// A renderer's overrides of the rule (per-renderer options, friendship_render_ext.h); the defaults are the measured best.
struct BankTuning {
    bool short_kernel = true;        // FR_BANK_SHORT
    uint64_t short_pairs = 1000;     // FR_SHORT_PAIRS: most (voice, tile) pairs the short-call kernel takes
    uint64_t short_wgs = 0;          // FR_SHORT_WGS: its workgroup target (0: the rule)
    uint32_t short_nw = 0;           // FR_SHORT_NW: its waves per workgroup (0: the rule)
    uint32_t bank_f = 0;             // FR_BANK_F: frames per lane of the time-major kernel (0: the rule)
    uint32_t bank_nw = 0;            // FR_BANK_NW: its waves per workgroup (0: the rule)
    bool multi = true;               // FR_BANK_MULTI=0: never the whole-voices-per-wave kernels for small voices
    uint32_t leaf_variant = 1;       // FR_BANK_LEAF=0: product-form leaves (BankArgs::leaf_variant)
    bool jit_chunks = true;          // FR_JIT_CHUNKS=0: compiled voices one workgroup per (voice, tile) always
    uint64_t jit_chunk_target = 0;   // FR_JIT_CHUNK_TARGET: workgroups below which a compiled voice is cut further (0: 1024, tracks 16384)
};

// The launch's call.
struct BankCall {
    uint64_t n_times = 0;            // window length
    bool host_pipelines = false;     // the call may overlap the previous one on another stream: no workspace shared between calls
    bool row_flags = false;          // the host entry point streams its output: the launch must publish row-completion flags
    bool jit_multi = false;          // jit groups: the compiled module has the whole-voices-per-wave entry
};

// One bank launch: the kernel and its shape (the BankArgs / JitBankArgs fields of the same names).
struct BankPlan {
    const char *kernel = "";         // fr_plan_json "bank_launches": bank_kernel, bank_multi_kernel, bank_small_kernel,
                                     // bank_short_kernel, gbank or jit_bank
    uint32_t chunk_log2 = 0;         // partials per workgroup (jit_bank: per piece; gbank: 0, whole voices)
    uint32_t frames_per_lane = 1, waves_per_group = 4, small_call = 0, voices_per_wave = 0;
    uint32_t pieces_log2 = 0;        // jit_bank: every voice rendered as 2^pieces_log2 pieces, added up by launch_chunk_combine
    uint64_t jit_blocks = 0;         // jit_bank: workgroups of the launch
    bool publishes_rows = false;     // with row_flags: the launch publishes them (time-major kernel, one chunk, FMA-form leaves)
    bool appends_rows = false;       // the launch can append a deferred input row to the history (BankArgs::hist_dst)
    uint64_t ws_floats = 0;          // workspace of the chunk (jit_bank: piece) sums, floats
    uint64_t ticket_words = 0;       // arrival counters of the short-call kernel's in-launch combine, words
};

// Many small voices, whole voices per wave (bank_multi_kernel, gbank_multi_kernel, jit_bank_multi): from `vpw` voices in a
// row, halved while the launch has fewer than 2048 workgroups of 4 waves; 0 if it still has fewer than 1024 (too few to
// fill the chip).
inline uint32_t whole_voices_per_wave(uint32_t vpw, uint32_t voices, uint64_t tiles) {
    auto nblocks = [&](uint32_t per_wave) { return ((voices + 4ull * per_wave - 1) / (4ull * per_wave)) * tiles; };
    while (vpw > 1 && nblocks(vpw) < 2048) vpw >>= 1;
    return nblocks(vpw) >= 1024 ? vpw : 0;
}

// The balanced hand-written kernels.  Measured on MI355X at 64 voices x 4096 partials
// (tools/bank_bench.hip, profiles/r01_bank_variants.txt, profiles/r01_bank_small_calls.txt):
//  * one 64-frame tile per wave (F = 1) is never slower than 2 or 4;
//  * long calls (>= 512 workgroups): 4 waves x 1024 partials per workgroup; 8 waves measured equal;
//  * short calls: ONE workgroup of 8 waves per (voice, tile) beats splitting voices into chunks + a combine
//    pass (T = 32: 13.9 us vs 31 us) and beats the lanes-over-partials kernel from T = 8 up (13.8 vs 17.4 us;
//    T = 32: 13.9 vs 37 us); lanes-over-partials only ties at T = 1 (11.4 us), so it is used for T <= 2;
//  * voices larger than one workgroup's capacity (8192 / 16384 partials) are split into chunks.
//  * the renderer's options (BankTuning) override parts of the rule for A/B runs: FR_BANK_SHORT=0 against the time-major
//    kernel, FR_SHORT_PAIRS / FR_SHORT_WGS / FR_SHORT_NW / FR_BANK_F / FR_BANK_NW.
// `many_pairs_whole`: do not cut a job of more than 320 (voice, tile) pairs into chunks (plan_bank: host_pipelines).
inline void bank_shape(uint32_t log2_p, uint32_t n_voices, uint64_t n_times, const BankTuning &tu, bool many_pairs_whole, BankPlan &p) {
    // short calls: few (voice, tile) pairs.  Chunks of >= 512 partials until there are ~256 workgroups of 16 waves.
    // Measured at 64 x 4096 (tools/short_call_probe.py, profiles/r02_short_calls.txt), us per call, this kernel vs the
    // time-major one: T <= 64: 7.4 vs 11.2; 128: 8.3 vs 11.4; 256: 10.6 vs 11.6; 512: 19.5 vs 17.8 -- hence pairs <= 320.
    // 512 or 1024 workgroups (more, smaller chunks) cost 2-3 us more in ticket traffic; 8 waves +0.3 us, 4 waves +2.4.
    const uint64_t pairs = ((n_times + 63) / 64) * n_voices;
    if (tu.short_kernel && pairs <= tu.short_pairs && log2_p >= 9 && log2_p <= 20 && pairs > 0) {
        // up to 320 pairs: ~256 workgroups of 16 waves; up to 1000 (a GPU's share of a voice-sharded job: 8 voices x 75
        // tiles): ~1200 workgroups of 8 waves -- 600 one-voice workgroups deal 2 or 3 to a CU (28 % idle), twice as
        // many half as long deal 4 or 5 (24.2 -> 21.9 us at 8 x 4096 x 4800; profiles/r02_short_calls.txt)
        const bool few = pairs <= 320;
        // (only where whole workgroups deal unevenly over the 256 CUs: 512 pairs are 2 per CU, and splitting them costs
        //  4 us of ticket traffic for nothing -- 17.7 -> 22.0 us at 64 x 4096 x 512)
        const bool lumpy = ((pairs + 255) / 256) * 256 * 100 >= pairs * 115;
        const uint64_t target = tu.short_wgs ? tu.short_wgs : (few ? 256ull : 1200ull);
        uint32_t c = log2_p;
        uint64_t wgs = pairs;
        while (c > 9 && (wgs < target || c > 13)) { --c; wgs *= 2; }
        if (log2_p - c <= 8 && (few || (lumpy && c != log2_p && !many_pairs_whole))) {
            p.chunk_log2 = c;
            p.waves_per_group = tu.short_nw ? tu.short_nw : (few ? 16u : 8u);
            while ((1u << c) / p.waves_per_group < 8u) p.waves_per_group /= 2;   // a wave needs a whole group of 8
            p.small_call = 2;
            return;
        }
    }
    if (n_times <= 2 && log2_p >= 8 && n_voices <= 65535u) {   // lanes over partials (only where the short-call kernel does not apply)
        p.small_call = 1;
        p.chunk_log2 = 8;
        return;
    }
    if (log2_p <= 8) {
        // many small voices: whole voices per wave (bank_multi_kernel).  Measured with tools/bank_bench at 4800 frames:
        // 4096 x 32 partials 2.1 -> 6.7 T partial-frames/s (8 voices in a row, 2 frames per lane), 1024 x 128 5.6 -> 8.2 and
        // 512 x 256 7.1 -> 8.5 (2 in a row); profiles/r01_small_and_silent_voices.txt.  Needs enough voices to fill the chip.
        const uint32_t F = (log2_p <= 5 && n_times >= 1024) ? 2u : 1u;
        const uint32_t vpw = whole_voices_per_wave(std::max(2u, 256u >> log2_p), n_voices, (n_times + 64 * F - 1) / (64 * F));
        if (vpw) {
            p.voices_per_wave = vpw;
            p.frames_per_lane = F;
            p.chunk_log2 = log2_p;
            return;
        }
    }
    const uint64_t blocks = ((n_times + 63) / 64) * n_voices;
    // small voices: a wave's share of the partials is a handful of groups, so the fixed cost per workgroup dominates;
    // 2 or 4 frames per lane amortise it (measured with tools/bank_bench: 32 partials 2.1 -> 3.2 T partial-frames/s,
    // 128 partials 5.3 -> 6.2, 512 partials 8.5 -> 8.8; at 4096 one frame per lane is best)
    if (n_times >= 1024 && blocks >= 4096) p.frames_per_lane = log2_p <= 7 ? 4 : (log2_p <= 9 ? 2 : 1);
    if (tu.bank_f == 1 || tu.bank_f == 2 || tu.bank_f == 4) p.frames_per_lane = tu.bank_f;   // A/B switch for measurements
    if (n_times >= 512 && blocks < 320 && log2_p >= 10) {
        // a few big voices on a long call: too few workgroups to hide the scalar-load latency of the parameter stream
        // (one 8-wave workgroup per tile leaves a SIMD with 1-2 waves).  Split the voices into chunks of >= 512 partials,
        // about 1024 workgroups in all, plus the combine pass (tools/bank_bench: 1 x 16384 at 4800 frames 25.7 -> 21.4 us,
        // 41 us with one 2^14 chunk; 4 x 4096 20.2 -> 17.8 us; at 512 frames 13.6 -> 11.2 us)
        uint32_t c = log2_p;
        uint64_t b2 = blocks;
        while (c > 9 && b2 < 1024) { --c; b2 *= 2; }
        p.chunk_log2 = c;
        p.frames_per_lane = 1;
        return;
    }
    // (64 x 4096 at 512 / 1024 frames, 512 / 1024 workgroups: 8 waves 20.7 / 32.3 us, 4 waves 23.4 / 35.5 us, chunks of 2^11 35 / 47 us)
    // (32 x 4096 x 4800, 2400 workgroups: 8 waves 65.2 us, 4 waves 66.9; 16 x 4096: 36.0 vs 38.5; 64 x 4096: equal)
    p.waves_per_group = (log2_p >= 14 || (blocks < 4096 && log2_p >= 6)) ? 8 : 4;
    if (tu.bank_nw == 4 && log2_p < 14) p.waves_per_group = 4;   // A/B
    if (tu.bank_nw == 8 && log2_p >= 6) p.waves_per_group = 8;
    const uint32_t cmax = p.waves_per_group == 8 ? 14 : 13;
    p.chunk_log2 = log2_p < cmax ? log2_p : cmax;
}

// The launch of bank group `g` in call `c` under the renderer's options `tu`.
// `n_voices`: the launch takes only that many of the group's voices (a run of them: engine.cpp's repair of kept delay lines).
inline BankPlan plan_bank(const BankLaunch &g, const BankCall &c, const BankTuning &tu, uint32_t n_voices = UINT32_MAX) {
    BankPlan p;
    const uint32_t voices = std::min<uint32_t>(n_voices, (uint32_t)g.rows.size());
    const uint64_t tiles = (c.n_times + 63) / 64;
    if (g.jit) {
        p.kernel = "jit_bank";
        if (tu.multi && g.log2_p <= 8 && c.jit_multi) p.voices_per_wave = whole_voices_per_wave(std::max(2u, 256u >> g.log2_p), voices, tiles);
        p.jit_blocks = tiles * (p.voices_per_wave ? (voices + 4ull * p.voices_per_wave - 1) / (4ull * p.voices_per_wave) : voices);
        // Few voices, short call: one workgroup per (voice, 64-frame tile) leaves most of the chip idle (64 voices x 64
        // frames = 64 workgroups).  Render every voice as 2^c consecutive pieces of its leaves instead -- to the kernel
        // 2^c times as many voices of 2^-c the size, rows of a workspace -- and add the pieces up in the tree's order.
        if (tu.jit_chunks && !g.to_ring && !g.to_ws && !p.voices_per_wave && voices <= 1024u) {
            // (voices that stream tracks from HBM want many small workgroups -- 64 x 4096 x 1024 frames: 0.84 of the achievable
            //  bandwidth with 1024 workgroups, 0.93 with 16 384; profiles/r03_tracks.txt -- the arithmetic-bound ones only a full chip)
            const uint64_t target = tu.jit_chunk_target ? tu.jit_chunk_target : (g.tracks ? 16384u : 1024u);
            while (p.pieces_log2 < 6 && g.log2_p - p.pieces_log2 > 5 && (p.jit_blocks << p.pieces_log2) < target) ++p.pieces_log2;
            // (T = 64: pieces of 256 partials beat 128 and 64 -- 34.5 / 37.3 / 35.3 us at 64 x 4096)
            if (g.tracks && c.n_times <= 128 && g.log2_p >= 8 && g.log2_p - p.pieces_log2 < 8) p.pieces_log2 = g.log2_p - 8;
        }
        const uint64_t pieces = (uint64_t)voices << p.pieces_log2;
        if (p.pieces_log2) { p.jit_blocks = tiles * pieces; p.ws_floats = pieces * c.n_times; }
        p.chunk_log2 = g.log2_p - p.pieces_log2;
        return p;
    }
    if (g.general) {   // many small voices: whole voices per wave (gbank_multi_kernel), like bank_multi_kernel for balanced ones
        p.kernel = "gbank";
        if (tu.multi && g.max_leaves <= 512)
            p.voices_per_wave = whole_voices_per_wave(std::max<uint32_t>(1u, std::min<uint32_t>(8u, 256u / std::max<uint32_t>(g.max_leaves, 1u))), voices, tiles);
        return p;
    }
    // (a host that renders ahead on alternating streams gets launches that can overlap: a GPU's share of a voice-sharded
    //  job, 8 x 4096 x 4800, takes 16.3 us per call that way against 20.9 with chunks + tickets on one stream -- the tail of
    //  one call's few latency-bound waves fills with the next call's first; profiles/r03_fewvoices.txt)
    bank_shape(g.log2_p, voices, c.n_times, tu, c.host_pipelines, p);
    if (p.voices_per_wave && !tu.multi) {   // A/B: the quarter-voice-per-wave kernel, one frame per lane
        p.voices_per_wave = 0;
        p.frames_per_lane = 1;
    }
    // small voices, many workgroups (one chunk, one frame per lane: as many as (voice, tile) pairs): ONE wave per (voice,
    // tile) -- no LDS combine, no barrier (256 x 512 x 4800: 71.6 -> 66.4 us; at 1024 partials and above 4 waves are as fast
    // or faster: profiles/r03_bank_waves.txt)
    if (g.log2_p <= 9 && g.log2_p >= 3 && p.chunk_log2 == g.log2_p && !p.small_call && !p.voices_per_wave && p.waves_per_group == 4 &&
        tu.leaf_variant == 1 && !c.row_flags && p.frames_per_lane == 1 && tiles * voices >= 4096)
        p.waves_per_group = 1;
    p.kernel = p.small_call == 2 ? "bank_short_kernel" : p.small_call ? "bank_small_kernel" : p.voices_per_wave ? "bank_multi_kernel" : "bank_kernel";
    // (only the time-major kernel with one chunk per voice and the FMA-form leaves publishes row flags into output rows;
    //  bank_small_kernel does not append history)
    p.publishes_rows = c.row_flags && !g.to_ring && !g.to_ws && !p.small_call && !p.voices_per_wave && tu.leaf_variant == 1 && p.chunk_log2 == g.log2_p;
    p.appends_rows = p.small_call != 1;
    if (p.chunk_log2 != g.log2_p) {
        p.ws_floats = ((uint64_t)voices << (g.log2_p - p.chunk_log2)) * c.n_times;
        if (p.small_call == 2) p.ticket_words = voices * tiles * BANK_TICKET_STRIDE;
    }
    return p;
}

// The kernel instance a launch of plan `p` runs, as one key (fr_plan_json "bank_launches" "variant"): the template arguments
// and the passes kernels.hip / jit.cpp pick for it.  `log2_p`: the group's; `leaf_variant`: BankTuning::leaf_variant;
// `row_flags`: BankCall::row_flags (the engine hands the launch the host's flags exactly then).  Mirrors the dispatch of
//   kernels.hip:999-1042 launch_bank: bank_short_kernel<NW> (its switch on waves_per_group, tickets when chunked),
//     bank_small_kernel and its bank_combine_kernel pass unless log2_p == 8, bank_multi_kernel<F, MODE> (MODE = leaf_variant
//     > 2 ? 1 : leaf_variant);
//   kernels.hip:972-997 launch_bank_f: bank_kernel<F, MODE, NW, FLAGS> -- FLAGS iff leaf_variant == 1 with host flags and one
//     chunk; NW 2 only for chunks <= 2^12, 1 only for chunks <= 2^11, else 4; MODE 2 always NW 4 -- and bank_combine_kernel
//     after a chunked launch;
//   kernels.hip:1335 launch_gbank: gbank_multi_kernel iff voices_per_wave;
//   jit.cpp:425 launch_jit_bank: jit_bank_multi iff voices_per_wave (plan_bank sets it only where the module has the entry),
//     and engine.cpp's launch_chunk_combine after a launch in pieces.
// tests/cpp/bankplan_sweep.cpp lists every key the rule can produce; tests/bank_variants.py has a GPU case for each.
inline std::string bank_variant(const BankPlan &p, uint32_t log2_p, uint32_t leaf_variant, bool row_flags) {
    const std::string k = p.kernel;
    if (k == "jit_bank") {
        if (p.voices_per_wave) return "jit_bank_multi";
        return p.pieces_log2 ? "jit_bank/pieces" + std::to_string(p.pieces_log2) : "jit_bank";
    }
    if (k == "gbank") return p.voices_per_wave ? "gbank_multi_kernel" : "gbank_kernel";
    if (k == "bank_short_kernel")
        return "bank_short_kernel<NW" + std::to_string(p.waves_per_group) + ">" + (p.chunk_log2 != log2_p ? "+tickets" : "");
    if (k == "bank_small_kernel") return std::string("bank_small_kernel") + (log2_p != 8 ? "+combine" : "");
    const std::string F = "F" + std::to_string(p.frames_per_lane);
    if (k == "bank_multi_kernel") return "bank_multi_kernel<" + F + ",M" + std::to_string(leaf_variant > 2 ? 1u : leaf_variant) + ">";
    const uint32_t w = p.waves_per_group;
    const bool flags = leaf_variant == 1 && row_flags && p.chunk_log2 == log2_p;
    uint32_t nw = 4;
    if (leaf_variant == 0 || flags) nw = w == 8 ? 8 : 4;
    else if (leaf_variant == 1) nw = w == 8 ? 8 : (w == 2 && p.chunk_log2 <= 12) ? 2 : (w == 1 && p.chunk_log2 <= 11) ? 1 : 4;
    const std::string mode = "M" + std::to_string(leaf_variant == 0 ? 0u : leaf_variant == 1 ? 1u : 2u);
    return "bank_kernel<" + F + "," + mode + ",NW" + std::to_string(nw) + (flags ? ",flags" : "") + ">" + (p.chunk_log2 != log2_p ? "+combine" : "");
}

}  // namespace fr
