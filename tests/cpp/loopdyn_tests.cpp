// loopdyn_tests.cpp -- FR_LOOP_DYN's plain logic on hand-built plans: W over mixed constant and signal reads (stage.hpp
// sweep_bound), the launch rule with every reason (callplan.hpp loop_sweep), what loop_tile answers a sweep plan, and a
// plain-loop model of the sweep form: for random amounts inside their proven ranges no frame of a sweep reads a frame of the
// same sweep.  Stand-alone: built and run on the CPU with -fsanitize=address,undefined by tests/test_loop_dyn_host.py.
#include <cstdio>
#include <random>
#include <string>

#include "../../libfriendship_amd/csrc/callplan.hpp"

using namespace fr;

static int passed = 0, failed = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (cond) ++passed;                                                         \
        else { ++failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

static StageInstr instr(uint8_t op, uint32_t buf = 0, uint32_t d_lo = 0, uint32_t imm = 0) {
    StageInstr in{};
    in.op = op;
    in.buf = buf;
    in.d_lo = d_lo;
    in.imm = imm;
    return in;
}

struct Read { bool dyn; uint32_t ring, lo, hi; };   // a constant read: lo = hi = d
// One merged program that stores `stores` with S_STOREs and reads `reads`.
static StageProg program(std::vector<StageInstr> &instrs, const std::vector<uint32_t> &stores, const std::vector<Read> &reads) {
    StageProg pg{};
    pg.first_instr = (uint32_t)instrs.size();
    pg.dst_ring = 0xFFFFFFFFu;
    pg.out_row = -1;
    instrs.push_back(instr(S_INPUT));
    for (const Read &r : reads) instrs.push_back(r.dyn ? instr(S_READ_DYN, r.ring, r.hi, r.lo) : instr(S_READ, r.ring, r.lo));
    for (uint32_t s : stores) instrs.push_back(instr(S_STORE, s));
    pg.n_instr = (uint32_t)instrs.size() - pg.first_instr;
    return pg;
}

static StagedPlan sweep_plan(uint64_t W) {
    StagedPlan sp;
    sp.feedback = true;
    sp.fused_sweep = W;
    sp.n_rings = 1;
    sp.progs.push_back(program(sp.instrs, {0}, {{true, 0, (uint32_t)W, (uint32_t)W + 6}}));
    sp.fused_first = 0;
    sp.fused_count = 1;
    sp.fused_level_first = {0, 1};
    return sp;
}

static void w_over_mixed_reads() {
    std::vector<StageInstr> ins;
    std::vector<StageProg> pgs;
    // no signal read of a program's ring at all: not a sweep plan, whatever the constants
    pgs.push_back(program(ins, {0}, {{false, 0, 5, 5}}));
    CHECK(sweep_bound(ins.data(), 0, pgs, {}) == 0);
    // ... nor when the only signal read is of a bank's ring
    pgs.push_back(program(ins, {1}, {{false, 1, 9, 9}, {true, 7, 0, 30}}));
    CHECK(sweep_bound(ins.data(), 0, pgs, {7}) == 0);
    // one signal read of an own ring: its floor(lo), against the constants of own rings -- the least wins
    pgs.push_back(program(ins, {2}, {{true, 2, 7, 14}}));
    CHECK(sweep_bound(ins.data(), 0, pgs, {7}) == 5);
    pgs[0] = program(ins, {0}, {{false, 0, 50, 50}});
    CHECK(sweep_bound(ins.data(), 0, pgs, {7}) == 7);
    // a merged two-node loop: a signal read in [5, 9] (bound 4) and a constant 3
    std::vector<StageInstr> ins2;
    std::vector<StageProg> two{program(ins2, {0, 1}, {{true, 1, 4, 9}, {false, 0, 3, 3}})};
    CHECK(sweep_bound(ins2.data(), 0, two, {}) == 3);
    // reads of rings an EARLIER level stores do not constrain W, even a signal read that may reach 0 frames back
    two.push_back(program(ins2, {2}, {{true, 0, 0, 3}, {false, 1, 1, 1}}));
    CHECK(sweep_bound(ins2.data(), 0, two, {}) == 3);
    // dst_ring counts as a store of the program
    std::vector<StageInstr> ins3;
    std::vector<StageProg> dst{program(ins3, {}, {{true, 4, 2, 5}})};
    dst[0].dst_ring = 4;
    CHECK(sweep_bound(ins3.data(), 0, dst, {}) == 2);
    // an instruction base other than 0 (the planner's fused instructions follow the level form's)
    std::vector<StageProg> shifted = dst;
    shifted[0].first_instr += 100;
    CHECK(sweep_bound(ins3.data(), 100, shifted, {}) == 2);
    // a signal read of an own ring with a proven bound of 0 frames: refused with the sentence such plans have always had
    std::vector<StageInstr> ins4;
    std::vector<StageProg> zero{program(ins4, {0}, {{false, 0, 5, 5}, {true, 0, 0, 3}})};
    bool threw = false;
    try { (void)sweep_bound(ins4.data(), 0, zero, {}); } catch (const Error &e) {
        threw = e.code == FR_ERR_UNSUPPORTED && has(e.what(), "a feedback plan reads a program's ring through a signal-dependent Delay");
    }
    CHECK(threw);
}

static void the_rule_and_every_reason() {
    StagedPlan none;   // no feedback: the option does not concern the plan
    for (int o = 0; o <= 2; ++o) {
        const LoopSweep ls = loop_sweep(none, o);
        CHECK(ls.form == LoopSweep::none && ls.sweep == 0 && ls.frames == 0 && ls.reason.empty() && std::string(ls.form_name()).empty());
    }
    StagedPlan strided;   // feedback through constant Delays
    strided.feedback = true;
    strided.fused_stride = 5;
    CHECK(loop_sweep(strided, 0).form == LoopSweep::none && loop_sweep(strided, 0).reason == "FR_LOOP_DYN is off");
    for (int o = 1; o <= 2; ++o) CHECK(loop_sweep(strided, o).form == LoopSweep::none && has(loop_sweep(strided, o).reason, "the strided form serves the plan"));
    for (uint64_t W : {1ull, 7ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 300ull, 2400ull, 1ull << 31}) {
        const StagedPlan sp = sweep_plan(W);
        const LoopSweep k = loop_sweep(sp, 1), w = loop_sweep(sp, 2);
        CHECK(k.form == LoopSweep::kernel && k.sweep == W && k.frames == std::min<uint64_t>(W, 256) && k.frames >= 1 && k.frames <= STAGE_SWEEP_MAX);
        CHECK(std::string(k.form_name()) == "sweep" && has(k.reason, ("at least " + std::to_string(W) + " frames back").c_str()));
        CHECK(w.form == LoopSweep::windows && w.sweep == W && w.frames == k.frames && std::string(w.form_name()) == "windows" && has(w.reason, "FR_LOOP_DYN=2"));
        CHECK(loop_sweep(sp, 0).form == LoopSweep::none && loop_sweep(sp, 0).reason == "FR_LOOP_DYN is off");
        // loop tiles: never, whatever FR_LOOP_TILES says, and the reason names the signal amount
        for (bool on : {false, true}) CHECK(loop_tile(sp, on).frames == 0 && has(loop_tile(sp, on).reason, "signal amount"));
    }
    CHECK(LOOP_SWEEP_MAX == STAGE_SWEEP_MAX);
}

// The sweep form as plain loops: x[t] = in[t] + 0.5 * x[t - a[t]], amounts a[t] drawn inside [lo, hi], sweeps of
// min(W, 256) frames with W = lo, the frames of a sweep in the least favourable order (last to first), each frame marked done
// only when its sweep has ended.  No read may touch a frame that is not done; the result must be the forward loop's.
static void no_frame_of_a_sweep_reads_its_own_sweep() {
    std::mt19937 rng(7);
    for (uint32_t lo : {1u, 2u, 7u, 63u, 64u, 65u, 255u, 256u, 257u, 300u}) {
        const uint32_t hi = lo + 1 + rng() % 40, n = 3000 + rng() % 500;
        const LoopSweep ls = loop_sweep(sweep_plan(lo), 1);
        std::vector<uint32_t> a(n);
        std::vector<float> in(n), fwd(n), x(n, 0.0f);
        std::vector<char> done(n, 0);
        for (uint32_t t = 0; t < n; ++t) { a[t] = lo + rng() % (hi - lo + 1); in[t] = (float)(rng() % 1000) / 250.0f - 2.0f; }
        a[10 % n] = lo; a[11 % n] = hi;                     // both ends of the range
        for (uint32_t t = 0; t < n; ++t) fwd[t] = in[t] + 0.5f * (t >= a[t] ? fwd[t - a[t]] : 0.0f);
        bool clean = true;
        for (uint32_t base = 0; base < n; base += ls.frames) {
            const uint32_t m = std::min<uint32_t>(ls.frames, n - base);
            for (uint32_t f = m; f-- > 0;) {
                const uint32_t t = base + f;
                float d = 0.0f;
                if (t >= a[t]) { clean = clean && done[t - a[t]]; d = x[t - a[t]]; }
                x[t] = in[t] + 0.5f * d;
            }
            for (uint32_t f = 0; f < m; ++f) done[base + f] = 1;   // the barrier
        }
        CHECK(clean);
        CHECK(x == fwd);
    }
    // and the bound is tight: one frame more per sweep than W does read its own sweep
    {
        const uint32_t W = 7, n = 200;
        std::vector<char> done(n, 0);
        bool clean = true;
        for (uint32_t base = 0; base < n; base += W + 1) {
            const uint32_t m = std::min<uint32_t>(W + 1, n - base);
            for (uint32_t f = m; f-- > 0;) if (base + f >= W) clean = clean && done[base + f - W];
            for (uint32_t f = 0; f < m; ++f) done[base + f] = 1;
        }
        CHECK(!clean);
    }
}

int main() {
    w_over_mixed_reads();
    the_rule_and_every_reason();
    no_frame_of_a_sweep_reads_its_own_sweep();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
