// streamplans.hpp -- the hand-built plans of the stand-alone streaming tests (streamlaunch_tests.cpp, streamcheck_tests.cpp): a
// staged plan, its bank launches and the options, assembled by hand, and for each resident kernel of the program path the
// smallest plan that calls for it (kernel_plan).
#pragma once

#include <cstdio>
#include <vector>

#include "../../libfriendship_amd/csrc/streamplan.hpp"

using namespace fr;

static int passed = 0, failed = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (cond) ++passed;                                                         \
        else { ++failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

constexpr uint32_t NO_RING = 0xFFFFFFFFu;

static StageInstr ins(uint8_t op, uint8_t dst, uint8_t a, uint8_t b, uint32_t imm, uint32_t buf, uint32_t d) {
    StageInstr i{};
    i.op = op; i.dst = dst; i.a = a; i.b = b; i.imm = imm; i.buf = buf; i.d_lo = d;
    return i;
}

struct Built {
    StagedPlan sp;
    std::vector<BankLaunch> banks;
    StreamEnv env;
    Built() { env.programs = true; }
    std::vector<const BankLaunch *> list() const {
        std::vector<const BankLaunch *> l;
        for (const BankLaunch &b : banks) l.push_back(&b);
        return l;
    }
    void bank(uint32_t log2_p, bool to_ring, std::vector<uint32_t> rows) {
        BankLaunch b;
        b.log2_p = log2_p;
        b.to_ring = to_ring;
        b.rows = std::move(rows);
        banks.push_back(b);
    }
    // a program of one level (a feedback plan: of the fused form)
    void program(const std::vector<StageInstr> &p, uint32_t result, uint32_t dst_ring, int32_t out_row) {
        StageProg pg{};
        pg.first_instr = (uint32_t)sp.instrs.size();
        pg.n_instr = (uint32_t)p.size();
        pg.result_reg = result;
        pg.dst_ring = dst_ring;
        pg.out_row = out_row;
        sp.instrs.insert(sp.instrs.end(), p.begin(), p.end());
        sp.progs.push_back(pg);
        sp.level_first = {0, (uint32_t)sp.progs.size()};
        if (sp.feedback) { sp.fused_first = 0; sp.fused_count = (uint32_t)sp.progs.size(); sp.post_first = sp.fused_count; }
    }
    StreamPlan plan() const { return plan_stream(sp, list(), env); }
};

// voice ring `ring` at the current frame to output row `row`
static std::vector<StageInstr> follow(uint32_t ring) { return {ins(S_READ, 0, 0, 0, 0, ring, 0)}; }
// x = voice ring + Delay(x, d), x in `ring` (a loop of d frames)
static std::vector<StageInstr> comb(uint32_t voice_ring, uint32_t ring, uint32_t d) {
    return {ins(S_READ, 0, 0, 0, 0, voice_ring, 0), ins(S_READ, 1, 0, 0, 0, ring, d), ins(S_SUM2, 0, 0, 1, 0, 0, 0), ins(S_STORE, 0, 0, 0, 0, ring, 0)};
}

// two voices of 128 partials behind rings 0 and 1, a program per voice that copies its ring to its row
static Built two_voices() {
    Built b;
    b.env.n_slots = 2;
    b.bank(7, true, {0, 1});
    b.sp.n_rings = 2;
    b.program(follow(0), 0, NO_RING, 0);
    b.program(follow(1), 0, NO_RING, 1);
    return b;
}

// The smallest plan that calls for kernel `k` of the program path (prog .. dyn).
static Built kernel_plan(StreamKernel k) {
    Built b = two_voices();
    switch (k) {
    case StreamKernel::prog:                                         // a program per voice
        break;
    case StreamKernel::bus:                                          // and a program that reads both voices of the block
        b.env.bus = true;
        b.env.n_slots = 3;
        b.program({ins(S_READ, 0, 0, 0, 0, 0, 0), ins(S_READ, 1, 0, 0, 0, 1, 0), ins(S_SUM2, 0, 0, 1, 0, 0, 0)}, 0, NO_RING, 2);
        break;
    case StreamKernel::in:                                           // a program reads slot 3 next to the time slot
        b.env.inputs = true;
        b.env.n_slots = 3;
        b.sp.input_slots = {0, 3};
        b.program({ins(S_INPUT, 0, 0, 0, 1, 0, 0)}, 0, NO_RING, 2);
        break;
    case StreamKernel::banks:                                        // a voice of 128 partials behind a program next to a voice of 512 that writes its row
        b = Built();
        b.env.n_slots = 2;
        b.env.banks = true;
        b.bank(7, true, {0});
        b.bank(9, false, {1});
        b.sp.n_rings = 1;
        b.program(follow(0), 0, NO_RING, 0);
        break;
    case StreamKernel::loops:                                        // a comb of 5 frames on voice 0
        b = Built();
        b.env.n_slots = 2;
        b.env.loops = true;
        b.bank(7, true, {0, 1});
        b.sp.feedback = true;
        b.sp.n_rings = 3;
        b.program(comb(0, 2, 5), 0, NO_RING, 0);
        b.program(follow(1), 0, NO_RING, 1);
        break;
    case StreamKernel::general:                                      // two voices of 32 partials that write their rows
        b = Built();
        b.env.n_slots = 2;
        b.env.general = true;
        b.bank(5, false, {0, 1});
        break;
    case StreamKernel::dyn:                                          // voice 0 delayed by a signal amount (the time row), voice 1 as it is
        b = Built();
        b.env.n_slots = 2;
        b.env.dyn = true;
        b.bank(7, true, {0, 1});
        b.sp.n_rings = 2;
        b.sp.input_slots = {0};
        b.program({ins(S_INPUT, 1, 0, 0, 0, 0, 0), ins(S_READ_DYN, 0, 1, 0, 0, 0, 20)}, 0, NO_RING, 0);
        b.program(follow(1), 0, NO_RING, 1);
        break;
    default:
        break;
    }
    return b;
}
