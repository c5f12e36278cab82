// looptile_tests.cpp -- the rule that decides whether a feedback plan's strided launches render tiles staged in LDS
// (libfriendship_amd/csrc/callplan.hpp loop_tile, FR_LOOP_TILES) on hand-built StagedPlans: the frames per tile of every
// stride, each refusal with its reason, the option off, a plan without feedback.  Stand-alone: built and run on the CPU with
// -fsanitize=address,undefined by tests/test_loop_tiles_host.py.
#include <cstdio>
#include <string>

#include "../../libfriendship_amd/csrc/callplan.hpp"

using namespace fr;

static int passed = 0, failed = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (cond) ++passed;                                                         \
        else { ++failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static StageInstr instr(uint8_t op, uint32_t imm = 0) {
    StageInstr in{};
    in.op = op;
    in.imm = imm;
    return in;
}

// x = in0 + c * Delay(x, stride), as the planner merges it: one fused program that stores its ring with a carry slot and
// reads it back through the slot, and a copy program after it.  `extra_loads` / `extra_stores` more of each in the loop.
static StagedPlan loop_plan(uint64_t stride, uint32_t extra_loads = 0, uint32_t extra_stores = 0) {
    StagedPlan sp;
    sp.feedback = true;
    sp.fused_carry_only = true;
    sp.fused_stride = stride;
    sp.n_rings = 1 + extra_stores;
    StageProg pg{};
    pg.first_instr = 0;
    pg.dst_ring = 0xFFFFFFFFu;
    pg.out_row = -1;
    sp.instrs.push_back(instr(S_INPUT, 0));
    sp.instrs.push_back(instr(S_READ, 1));         // the carry's slot 0
    sp.instrs.push_back(instr(S_CONST, 0x3F000000u));
    sp.instrs.push_back(instr(S_MUL));
    sp.instrs.push_back(instr(S_SUM2));
    for (uint32_t i = 0; i < extra_loads; ++i) sp.instrs.push_back(instr(i % 3 == 0 ? S_INPUT : i % 3 == 1 ? S_READ_INPUT : S_READ, 0));
    sp.instrs.push_back(instr(S_STORE, 1));
    for (uint32_t i = 0; i < extra_stores; ++i) sp.instrs.push_back(instr(S_STORE, i + 2 <= 8 ? i + 2 : 0));
    pg.n_instr = (uint32_t)sp.instrs.size();
    sp.progs.push_back(pg);
    sp.fused_first = 0;
    sp.fused_count = 1;
    sp.fused_level_first = {0, 1};
    StageProg copy{};   // ring 0 -> row 0: not a fused program, the rule does not look at it
    copy.first_instr = (uint32_t)sp.instrs.size();
    copy.n_instr = 1;
    copy.dst_ring = 0xFFFFFFFFu;
    copy.out_row = 0;
    sp.instrs.push_back(instr(S_READ, 0));
    sp.progs.push_back(copy);
    sp.post_first = 1;
    sp.post_count = 1;
    return sp;
}

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

static void frames_of_every_stride() {
    // every stride the kernels could take (a lane per residue): tiled up to LOOP_TILE_MAX_STRIDE -- set by measurement --, refused
    // with the stride's reason above it
    CHECK(LOOP_TILE_MAX_STRIDE >= 1 && LOOP_TILE_MAX_STRIDE <= 64);
    for (uint64_t d = 1; d <= 64; ++d) {
        const LoopTile lt = loop_tile(loop_plan(d), true);
        const uint64_t frames = d * (256 / d);
        CHECK(frames % d == 0 && frames <= 256 && frames + d > 256);   // the largest multiple of the stride in a tile
        if (d <= LOOP_TILE_MAX_STRIDE) CHECK(lt.frames == frames && lt.reason.empty());
        else CHECK(lt.frames == 0 && has(lt.reason, ("stride is " + std::to_string(d) + " frames").c_str()));
    }
    const uint32_t pinned[][2] = {{1, 256}, {2, 256}, {3, 255}, {5, 255}, {7, 252}, {16, 256}, {33, 231}, {64, 256}};
    for (const auto &pf : pinned)
        if (pf[0] <= LOOP_TILE_MAX_STRIDE) CHECK(loop_tile(loop_plan(pf[0]), true).frames == pf[1]);
    CHECK(LOOP_TILE_FRAMES == STAGE_TILE_FRAMES && LOOP_TILE_LOADS == STAGE_TILE_LOADS && LOOP_TILE_STORES == STAGE_TILE_STORES);
}

static void refusals() {
    LoopTile lt = loop_tile(loop_plan(65), true);
    CHECK(lt.frames == 0 && has(lt.reason, "stride is 65"));
    lt = loop_tile(loop_plan(0), true);
    CHECK(lt.frames == 0 && has(lt.reason, "stride is 0"));
    lt = loop_tile(loop_plan(2400), true);
    CHECK(lt.frames == 0 && has(lt.reason, "stride is 2400"));
    {
        StagedPlan sp = loop_plan(2);   // a tap two strides back: read through memory
        sp.fused_carry_only = false;
        sp.instrs[1].imm = 0xFFu;
        lt = loop_tile(sp, true);
        CHECK(lt.frames == 0 && lt.reason == "a loop reads its own ring further back than one stride");
    }
    // loads: the program has 1; 15 more fit, the 17th does not.  The carry's read is no load.
    CHECK(loop_tile(loop_plan(5, 15), true).frames == 255);
    lt = loop_tile(loop_plan(5, 16), true);
    CHECK(lt.frames == 0 && has(lt.reason, "fused program 0 has 17 frame-only loads"));
    // stores: 1 S_STORE; 11 more fit
    CHECK(loop_tile(loop_plan(5, 0, 11), true).frames == 255);
    lt = loop_tile(loop_plan(5, 0, 12), true);
    CHECK(lt.frames == 0 && has(lt.reason, "fused program 0 has 13 stores"));
    {
        StagedPlan sp = loop_plan(5, 0, 10);   // dst_ring and out_row count as stores
        sp.progs[0].dst_ring = 7;
        CHECK(loop_tile(sp, true).frames == 255);
        sp.progs[0].out_row = 3;
        lt = loop_tile(sp, true);
        CHECK(lt.frames == 0 && has(lt.reason, "has 13 stores"));
    }
    for (uint8_t op : {(uint8_t)S_READ_DYN, (uint8_t)S_READ_INPUT_DYN, (uint8_t)S_STEP_DYN}) {
        StagedPlan sp = loop_plan(4);
        sp.instrs[2].op = op;
        lt = loop_tile(sp, true);
        CHECK(lt.frames == 0 && has(lt.reason, "fused program 0 delays by a signal amount"));
    }
    {
        StagedPlan sp = loop_plan(4);   // the copy program is not looked at
        sp.instrs[sp.progs[1].first_instr].op = S_READ_DYN;
        CHECK(loop_tile(sp, true).frames == 256);
    }
}

static void off_and_no_feedback() {
    for (uint64_t d : {1, 3, 16, 64, 65}) {
        const LoopTile lt = loop_tile(loop_plan(d), false);
        CHECK(lt.frames == 0 && lt.reason == "FR_LOOP_TILES is off");
    }
    StagedPlan sp = loop_plan(1);
    sp.feedback = false;   // (a strided effects chain: the non-feedback strided form is never tiled)
    CHECK(loop_tile(sp, true).frames == 0 && loop_tile(sp, true).reason.empty());
    CHECK(loop_tile(sp, false).frames == 0 && loop_tile(sp, false).reason.empty());
    CHECK(loop_tile(StagedPlan{}, true).frames == 0);
}

int main() {
    frames_of_every_stride();
    refusals();
    off_and_no_feedback();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
