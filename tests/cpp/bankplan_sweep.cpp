// bankplan_sweep.cpp -- every kernel instance the bank launch rule (csrc/bankplan.hpp plan_bank, bank_variant) can pick.
// Sweeps plan_bank over group kinds (balanced, general, compiled with and without tracks), sizes, call lengths, every
// BankTuning override and their combinations, host_pipelines and row_flags, and prints the set of variant keys, each with
// the first grid point that reaches it:  <key>\t<point>.  tests/test_bank_variants.py compares the set with the GPU case
// table (tests/bank_variants.py).
//
// `--query`: reads one launch per line from stdin and prints its key, its number of workgroups and its
// voices per wave, so that a test can check on the CPU that each GPU
// case's shape and options reach the key the case is named after:
//   kind log2_p voices max_leaves tracks jit_multi n_times host_pipelines row_flags
//   short_kernel short_pairs short_wgs short_nw bank_f bank_nw multi leaf_variant jit_chunks jit_chunk_target
// (kind: 0 balanced, 1 compiled, 2 general).
//
// `--tracks`: the same sweep over the groups that stream tracks only (compiled voices with `tracks` set), in the same
// format: the keys tests/track_variants.py must cover (tests/test_track_variants.py).
//
// Build: g++ -std=c++17 -O2 -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -o bankplan_sweep bankplan_sweep.cpp
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../libfriendship_amd/csrc/bankplan.hpp"

using namespace fr;

namespace {

enum Kind { BAL, JIT, GEN };

BankPlan launch(Kind kind, uint32_t log2_p, uint32_t voices, uint32_t max_leaves, bool tracks, bool jit_multi, uint64_t n_times,
               bool host_pipelines, bool row_flags, const BankTuning &tu) {
    static BankLaunch g;   // (reused: the rule reads only the number of rows)
    g.log2_p = log2_p;
    g.rows.resize(voices);
    g.max_leaves = max_leaves;
    g.jit = kind == JIT;
    g.general = kind == GEN;
    g.tracks = tracks;
    return plan_bank(g, BankCall{n_times, host_pipelines, row_flags, jit_multi}, tu);
}

// Everything bank_variant reads, packed: the sweep builds the key string only for a combination not met before.
uint64_t pack(const BankPlan &p, uint32_t log2_p, uint32_t leaf_variant, bool row_flags) {
    return (uint64_t)std::strlen(p.kernel) | (uint64_t)p.chunk_log2 << 8 | (uint64_t)log2_p << 16 | (uint64_t)p.frames_per_lane << 24 |
           (uint64_t)p.waves_per_group << 28 | (uint64_t)(p.voices_per_wave ? 1 : 0) << 36 | (uint64_t)p.pieces_log2 << 40 |
           (uint64_t)leaf_variant << 48 | (uint64_t)row_flags << 56 | (uint64_t)p.small_call << 60;   // (small_call: kernel names of one length)
}

int query() {
    unsigned kind, log2_p, voices, max_leaves, tracks, jit_multi, hp, rf, sk, snw, bf, bnw, multi, leaf, jc;
    unsigned long long n_times, sp, swgs, jt;
    while (std::cin >> kind >> log2_p >> voices >> max_leaves >> tracks >> jit_multi >> n_times >> hp >> rf >> sk >> sp >> swgs >> snw >> bf >>
           bnw >> multi >> leaf >> jc >> jt) {
        BankTuning tu;
        tu.short_kernel = sk;
        tu.short_pairs = sp;
        tu.short_wgs = swgs;
        tu.short_nw = snw;
        tu.bank_f = bf;
        tu.bank_nw = bnw;
        tu.multi = multi;
        tu.leaf_variant = leaf;
        tu.jit_chunks = jc;
        tu.jit_chunk_target = jt;
        const BankPlan p = launch((Kind)kind, log2_p, voices, max_leaves, tracks, jit_multi, n_times, hp, rf, tu);
        // and its workgroups (kernels.hip launch_bank_short / launch_bank_f / the multi and small branches of launch_bank,
        // launch_gbank; jit_bank: jit_blocks)
        const uint64_t F = p.frames_per_lane, tiles = (n_times + 64 * F - 1) / (64 * F);
        uint64_t blocks = p.voices_per_wave ? tiles * ((voices + 4ull * p.voices_per_wave - 1) / (4ull * p.voices_per_wave))
                                            : (tiles * voices) << (log2_p - p.chunk_log2);
        if (p.small_call == 1) blocks = (uint64_t)voices << (log2_p - 8);
        if (kind == JIT) blocks = p.jit_blocks;
        std::printf("%s %llu %u\n", bank_variant(p, log2_p, tu.leaf_variant, rf).c_str(), (unsigned long long)blocks, p.voices_per_wave);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && std::strcmp(argv[1], "--query") == 0) return query();
    const bool tracks_only = argc > 1 && std::strcmp(argv[1], "--tracks") == 0;
    // voices 1 .. 4096 and frames 1 .. 8192: every threshold of the rule (64-frame tiles, 320 / 1000 pairs, 1024 / 2048 / 4096
    // workgroups, 512 / 1024 frames, the 2-frame small call) lies between two neighbours of these lists
    const std::vector<uint32_t> voice_counts = {1, 2, 3, 4, 5, 7, 8, 12, 16, 31, 64, 100, 128, 255, 256, 257, 400, 512, 700, 1000, 1024, 1025, 2000, 4096};
    const std::vector<uint64_t> frame_counts = {1, 2, 3, 63, 64, 65, 100, 128, 129, 200, 256, 300, 511, 512, 640, 1000, 1023, 1024, 1100, 2048, 4096, 4800, 8192};
    const std::vector<uint32_t> leaf_counts = {1, 3, 8, 20, 64, 100, 256, 512, 513, 600, 2000};   // general voices' largest
    std::map<std::string, std::string> keys;
    std::unordered_set<uint64_t> seen;
    uint64_t points = 0;
    auto note = [&](Kind k, const char *kind, uint32_t log2_p, uint32_t voices, uint32_t leaves, bool tracks, bool jm, uint64_t T, bool hp, bool rf,
                    const BankTuning &tu) {
        if (tracks_only && !tracks) return;
        ++points;
        const BankPlan p = launch(k, log2_p, voices, leaves, tracks, jm, T, hp, rf, tu);
        if (!seen.insert(pack(p, log2_p, tu.leaf_variant, rf)).second) return;
        const std::string key = bank_variant(p, log2_p, tu.leaf_variant, rf);
        if (keys.count(key)) return;
        char buf[512];
        std::snprintf(buf, sizeof buf,
                      "%s log2_p=%u voices=%u max_leaves=%u tracks=%d jit_multi=%d n_times=%llu host_pipelines=%d row_flags=%d | short=%d "
                      "pairs=%llu wgs=%llu snw=%u F=%u NW=%u multi=%d leaf=%u jit_chunks=%d target=%llu",
                      kind, log2_p, voices, leaves, tracks, jm, (unsigned long long)T, hp, rf, tu.short_kernel, (unsigned long long)tu.short_pairs,
                      (unsigned long long)tu.short_wgs, tu.short_nw, tu.bank_f, tu.bank_nw, tu.multi, tu.leaf_variant, tu.jit_chunks,
                      (unsigned long long)tu.jit_chunk_target);
        keys[key] = buf;
    };
    // every combination of the balanced kernels' overrides (FR_BANK_SHORT, FR_SHORT_PAIRS, FR_SHORT_WGS, FR_SHORT_NW, FR_BANK_F,
    // FR_BANK_NW, FR_BANK_MULTI, FR_BANK_LEAF; options outside the accepted values are refused at renderer creation)
    std::vector<BankTuning> bal_tunes;
    for (bool sk : {true, false})
        for (uint64_t sp : {1000ull, 200ull, 4000ull})
            for (uint64_t swgs : {0ull, 64ull, 512ull, 4096ull})
                for (uint32_t snw : {0u, 4u, 8u, 16u})
                    for (uint32_t bf : {0u, 1u, 2u, 4u})
                        for (uint32_t bnw : {0u, 4u, 8u})
                            for (bool multi : {true, false})
                                for (uint32_t leaf : {1u, 0u}) {
                                    BankTuning t;
                                    t.short_kernel = sk;
                                    t.short_pairs = sp;
                                    t.short_wgs = swgs;
                                    t.short_nw = snw;
                                    t.bank_f = bf;
                                    t.bank_nw = bnw;
                                    t.multi = multi;
                                    t.leaf_variant = leaf;
                                    bal_tunes.push_back(t);
                                }
    // the compiled and general voices' overrides (FR_BANK_MULTI, FR_JIT_CHUNKS, FR_JIT_CHUNK_TARGET)
    std::vector<BankTuning> jit_tunes;
    for (bool multi : {true, false})
        for (bool jc : {true, false})
            for (uint64_t target : {0ull, 2ull, 8ull, 64ull, 1024ull, 65536ull}) {
                BankTuning t;
                t.multi = multi;
                t.jit_chunks = jc;
                t.jit_chunk_target = target;
                jit_tunes.push_back(t);
            }
    for (uint32_t log2_p = 0; log2_p <= 16; ++log2_p)
        for (uint32_t V : voice_counts)
            for (uint64_t T : frame_counts)
                for (bool hp : {false, true})
                    for (bool rf : {false, true}) {
                        // balanced template voices: 2^5 leaves and more (match.cpp BankMatcher::match); compiled voices: 2^5 .. 2^13
                        // (match_shape_voice); general voices: any tree, log2_p unused
                        if (log2_p >= 5)
                            for (const BankTuning &tu : bal_tunes) note(BAL, "balanced", log2_p, V, 0, false, false, T, hp, rf, tu);
                        if (log2_p >= 5 && log2_p <= 13)
                            for (const BankTuning &tu : jit_tunes)
                                for (bool tracks : {false, true})
                                    for (bool jm : {false, true})
                                        note(JIT, "jit", log2_p, V, 0, tracks, jm, T, hp, rf, tu);
                        if (log2_p == 0)
                            for (uint32_t L : leaf_counts)
                                for (const BankTuning &tu : jit_tunes) note(GEN, "general", 0, V, L, false, false, T, hp, rf, tu);
                    }
    for (const auto &kv : keys) std::printf("%s\t%s\n", kv.first.c_str(), kv.second.c_str());
    std::printf("%zu keys over %llu launches\n", keys.size(), (unsigned long long)points);
    return 0;
}
