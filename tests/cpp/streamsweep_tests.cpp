// streamsweep_tests.cpp -- FR_STREAM_SWEEP on the host (libfriendship_amd/csrc/streamplan.hpp, kernels.hpp): the width and the
// slot-marking helper on hand-built programs (the edges 63 / 64, a bound of 0, the tiles' limits), the serving rule and the launch
// rule on hand-built plans -- each new admission and each refusal that survives --, the form and the launch check of the four
// sweep kernels, and a plain-loop model of the sweep walk (kernels.hip stream_run_loop_program<true>) run on the helper's output
// and compared bit for bit with a frame-by-frame evaluation of the plan's own instructions, amounts random inside their proven
// intervals, blocks of 1..64 frames (n < w included), widths 1, 7 and 63.  Stand-alone: built and run on the CPU with
// -fsanitize=address,undefined by tests/test_stream_sweep_host.py.
#include <cmath>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "streamplans.hpp"

static uint32_t f32(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }
static float bitsf(uint32_t u) { float v; std::memcpy(&v, &u, 4); return v; }

static StageProg prog(const std::vector<StageInstr> &p, uint32_t result, uint32_t dst_ring, int32_t out_row) {
    StageProg pg{};
    pg.n_instr = (uint32_t)p.size();
    pg.result_reg = result;
    pg.dst_ring = dst_ring;
    pg.out_row = out_row;
    return pg;
}

static const char *const OLD_SWEEP = "a feedback loop delays by a signal amount (a sweep plan, FR_LOOP_DYN): block streaming does not serve it";
static const char *const OLD_LOOP_DYN = "a loop program uses S_READ_DYN (a Delay by a signal amount inside a feedback loop shorter than a block), which block streaming does not serve yet";
static const char *const OLD_DYN_RING = "a program uses S_READ_DYN of a ring that a program stores (a Delay of a computed value by a signal amount, which may be 0 "
                                        "frames); block streaming serves signal delays of voices only";

// x = src + 0.5 * Delay(x, amount), amount = input row `amt_row` (bound `lo` .. `hi` frames), x in `ring`; src: ring `src_ring` at
// the current frame, or input row 0 when src_ring is NO_RING.  `store`: an explicit S_STORE (else the caller gives dst_ring).
static std::vector<StageInstr> flanger(uint32_t src_ring, uint32_t ring, uint32_t amt_row, uint32_t lo, uint32_t hi, bool store) {
    std::vector<StageInstr> p;
    p.push_back(src_ring == NO_RING ? ins(S_INPUT, 0, 0, 0, 0, 0, 0) : ins(S_READ, 0, 0, 0, 0, src_ring, 0));
    p.push_back(ins(S_INPUT, 3, 0, 0, amt_row, 0, 0));
    p.push_back(ins(S_READ_DYN, 1, 3, 0, lo, ring, hi));
    p.push_back(ins(S_CONST, 2, 0, 0, f32(0.5f), 0, 0));
    p.push_back(ins(S_MUL, 1, 1, 2, 0, 0, 0));
    p.push_back(ins(S_SUM2, 0, 0, 1, 0, 0, 0));
    if (store) p.push_back(ins(S_STORE, 0, 0, 0, 9u, ring, 0));
    return p;
}

static void test_helpers() {
    {   // a flanger of bound 7: width 7; the store slot replaces the bound
        std::vector<StageInstr> p = flanger(0, 1, 1, 7, 14, true);
        StageProg pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_sweep_width(pg, p.data()) == 7 && stream_loop_stride(pg, p.data()) == 0);
        CHECK(stream_sweep_prepare(pg, p));
        CHECK(pg.pad[0] == 7 && pg.n_instr == p.size() && pg.dst_ring == NO_RING);
        CHECK(p[0].imm == 0 && p[2].op == S_READ_DYN && p[2].imm == 1 && p[2].d_lo == 14 && p.back().op == S_STORE && p.back().imm == 1);
    }
    {   // the same through dst_ring: the helper appends the store
        std::vector<StageInstr> p = flanger(NO_RING, 4, 1, 2, 5, false);
        StageProg pg = prog(p, 0, 4, 3);
        CHECK(stream_sweep_width(pg, p.data()) == 2);
        CHECK(stream_sweep_prepare(pg, p));
        CHECK(pg.pad[0] == 2 && pg.n_instr == 7 && p.size() == 7 && pg.dst_ring == NO_RING && pg.out_row == 3);
        CHECK(p[6].op == S_STORE && p[6].buf == 4 && p[6].a == 0 && p[6].imm == 1 && p[2].imm == 1);
    }
    for (uint32_t lo : {1u, 2u, 62u, 63u}) {   // the edges below a block
        std::vector<StageInstr> p = flanger(0, 1, 1, lo, 100, true);
        StageProg pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_sweep_width(pg, p.data()) == lo && stream_sweep_prepare(pg, p) && pg.pad[0] == lo);
    }
    for (uint32_t lo : {64u, 65u, 1000u}) {    // no read reaches into a block: 64, and nothing to prepare
        std::vector<StageInstr> p = flanger(0, 1, 1, lo, 2000, true);
        const std::vector<StageInstr> before = p;
        StageProg pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_sweep_width(pg, p.data()) == 64 && !stream_sweep_prepare(pg, p) && pg.pad[0] == 0);
        CHECK(std::memcmp(before.data(), p.data(), p.size() * sizeof(StageInstr)) == 0);
    }
    {   // a bound of 0: no width, nothing the kernel may run
        std::vector<StageInstr> p = flanger(0, 1, 1, 0, 10, true);
        StageProg pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_sweep_width(pg, p.data()) == 0 && !stream_sweep_prepare(pg, p));
    }
    {   // no own-ring S_READ_DYN: a constant comb is no sweep program, nor is a program that delays ANOTHER ring by a signal amount
        std::vector<StageInstr> p = comb(0, 1, 5);
        StageProg pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_sweep_width(pg, p.data()) == 0 && !stream_sweep_prepare(pg, p) && stream_loop_stride(pg, p.data()) == 5);
        p = comb(0, 1, 5);
        p.insert(p.begin(), {ins(S_INPUT, 3, 0, 0, 1, 0, 0), ins(S_READ_DYN, 4, 3, 0, 3, 0, 9)});
        pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_sweep_width(pg, p.data()) == 0 && !stream_sweep_prepare(pg, p));
    }
    {   // a constant tap below the bound is the width, one above it is not; taps of a block or more do not count
        std::vector<StageInstr> p = flanger(0, 1, 1, 5, 9, false);
        p.push_back(ins(S_READ, 4, 0, 0, 0xEEu, 1, 3));
        p.push_back(ins(S_READ, 5, 0, 0, 0xEEu, 1, 200));
        p.push_back(ins(S_READ_DYN, 6, 3, 0, 77, 0, 90));            // the voice's ring by a signal amount: its imm is cleared
        p.push_back(ins(S_STORE, 0, 0, 0, 0, 1, 0));
        StageProg pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_sweep_width(pg, p.data()) == 3);
        CHECK(stream_sweep_prepare(pg, p) && pg.pad[0] == 3);
        CHECK(p[2].imm == 1 && p[6].imm == 1 && p[7].imm == 1 && p[8].imm == 0 && p[0].imm == 0);
        p[6].d_lo = 12;
        pg = prog(p, 0, NO_RING, 0);
        p[2].imm = 5;
        CHECK(stream_sweep_width(pg, p.data()) == 5);
    }
    {   // two stored rings (a merged circle): slots in store order, the own S_READ_DYN marked with its ring's slot
        std::vector<StageInstr> p{ins(S_INPUT, 0, 0, 0, 0, 0, 0), ins(S_INPUT, 3, 0, 0, 1, 0, 0), ins(S_READ_DYN, 1, 3, 0, 4, 2, 9), ins(S_SUM2, 0, 0, 1, 0, 0, 0),
                                  ins(S_STORE, 0, 0, 0, 0, 1, 0), ins(S_READ, 2, 0, 0, 0, 1, 3), ins(S_STORE, 0, 2, 0, 0, 2, 0)};
        StageProg pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_sweep_width(pg, p.data()) == 3 && stream_sweep_prepare(pg, p) && pg.pad[0] == 3);
        CHECK(p[2].imm == 2 && p[4].imm == 1 && p[5].imm == 1 && p[6].imm == 2);
    }
    {   // the tiles' limits: 17 stored rings, 33 loads
        std::vector<StageInstr> p = flanger(0, 1, 1, 7, 14, true);
        for (uint32_t r = 0; r < STREAM_LOOP_STORES; ++r) p.push_back(ins(S_STORE, 0, 0, 0, 0, 10 + r, 0));
        StageProg pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_sweep_width(pg, p.data()) == 7 && !stream_sweep_prepare(pg, p));
        p.pop_back();
        pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_sweep_prepare(pg, p) && p.back().imm == STREAM_LOOP_STORES);
        p = flanger(0, 1, 1, 7, 14, true);                             // two loads; _DYN ops take no slot
        for (uint32_t k = 0; k < STREAM_LOOP_LOADS - 1; ++k) p.insert(p.begin(), ins(S_READ, 7, 0, 0, 0, 0, 100 + k));
        pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_loop_loads(pg, p.data()) == STREAM_LOOP_LOADS + 1 && !stream_sweep_prepare(pg, p));
        p.erase(p.begin());
        pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_loop_loads(pg, p.data()) == STREAM_LOOP_LOADS && stream_sweep_prepare(pg, p));
        std::vector<StageInstr> q = flanger(0, 1, 1, 7, 14, true);
        pg = prog(q, 0, NO_RING, 0);
        q.pop_back();                                                  // (a copy that is not the program's)
        CHECK(!stream_sweep_prepare(pg, q));
    }
}

// ---- the rule and the launch rule on hand-built plans -------------------------------------------------------------------------
// two voices behind rings 0 and 1, a flanger of bound `lo` on each (rings 2 and 3): a sweep plan with voices
static Built voices_plan(uint32_t lo, uint32_t hi = 14) {
    Built b;
    b.env.n_slots = 2;
    b.env.loops = b.env.dyn = b.env.sweep = true;
    b.bank(7, true, {0, 1});
    b.sp.feedback = true;
    b.sp.fused_sweep = lo;
    b.sp.n_rings = 4;
    b.sp.input_slots = {0};
    b.program(flanger(0, 2, 0, lo, hi, true), 0, NO_RING, 0);
    b.program(flanger(1, 3, 0, lo, hi, true), 0, NO_RING, 1);
    return b;
}
// no voice: a flanger on input row 0 whose amount is row 1 (slot 1), ring 0
static Built voiceless_plan(uint32_t lo, uint32_t hi = 14) {
    Built b;
    b.env.n_slots = 1;
    b.env.loops = b.env.dyn = b.env.sweep = b.env.effects = b.env.inputs = true;
    b.sp.feedback = true;
    b.sp.fused_sweep = lo;
    b.sp.n_rings = 1;
    b.sp.input_slots = {0, 1};
    b.program(flanger(NO_RING, 0, 1, lo, hi, true), 0, NO_RING, 0);
    return b;
}

static void test_rule() {
    {   // (a) with voices: width 7 where the stride stands; the sweep form of the hist kernel
        const Built b = voices_plan(7);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.reason.empty());
        CHECK(s.loop_stride == (std::vector<uint32_t>{7, 7}) && s.sweep_width == (std::vector<uint32_t>{7, 7}) && s.has_sweep() && s.has_loops() && !s.sweep_loops);
        CHECK(s.min_ring_delay == 7 && s.lookback == 14 && s.dyn_reads == 2 && s.dyn_ring_reads == 2 && s.short_reads == 2 && s.dyn_steps == 0);
        CHECK(s.voice_first == (std::vector<uint32_t>{0, 1, 2, 2}));
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(l.kernel == StreamKernel::sweep && std::string(stream_kernel_name(l.kernel)) == "bank_stream_sweep_kernel");
        CHECK(l.rows_doorbell && l.own_instrs && l.by_plan && l.bank_table && !l.schedule_table && l.hist_cap == 64 && l.n_rows == 1);
        CHECK(l.max_stride == 7 && l.max_loads == 2 && l.max_stores == 1 && l.workgroups == 2);
        Built st = b;
        st.env.store = true;
        const StreamPlan t = st.plan();
        CHECK(t.servable && stream_launch(st.sp, t).kernel == StreamKernel::sweep_store && stream_launch(st.sp, t).hist_cap == 64);
    }
    {   // (a) without a voice: the sweep form of the fx kernel, and of store_fx
        const Built b = voiceless_plan(1, 5);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.voices == 0 && s.segments == 1 && s.sweep_width == (std::vector<uint32_t>{1}) && s.loop_stride == (std::vector<uint32_t>{1}));
        CHECK(s.min_ring_delay == 1 && s.lookback == 5 && s.input_slots == (std::vector<uint32_t>{0, 1}));
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(l.kernel == StreamKernel::sweep_fx && !l.bank_table && !l.schedule_table && l.hist_cap == 64 && l.n_rows == 2 && l.workgroups == 1 && l.max_stride == 1);
        Built st = b;
        st.env.store = true;
        CHECK(stream_launch(st.sp, st.plan()).kernel == StreamKernel::sweep_store_fx);
    }
    for (uint32_t lo : {63u, 64u}) {   // the edge: 63 is the widest sweep; at 64 the program runs lane = frame and the plan keeps its kernel
        const Built b = voiceless_plan(lo, 70);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.min_ring_delay == lo && s.dyn_reads == 1 && s.dyn_ring_reads == 1 && s.short_reads == (lo < 64 ? 1u : 0u));
        CHECK(s.sweep_width == (std::vector<uint32_t>{lo < 64 ? lo : 0u}) && s.loop_stride == s.sweep_width && s.has_sweep() == (lo < 64));
        CHECK(stream_launch(b.sp, s).kernel == (lo < 64 ? StreamKernel::sweep_fx : StreamKernel::fx));
        const Built v = voices_plan(lo, 70);
        CHECK(stream_launch(v.sp, v.plan()).kernel == (lo < 64 ? StreamKernel::sweep : StreamKernel::dyn));
    }
    {   // the option, or one it acts on top of, missing: today's sentence word for word
        for (int missing = 0; missing < 3; ++missing) {
            Built b = voices_plan(7);
            (missing == 0 ? b.env.sweep : missing == 1 ? b.env.loops : b.env.dyn) = false;
            const StreamPlan s = b.plan();
            CHECK(!s.servable && s.reason == OLD_SWEEP && s.progs.empty() && s.sweep_width.empty());
        }
        Built b = voiceless_plan(7);
        b.env.sweep = false;
        CHECK(b.plan().reason == OLD_SWEEP);
    }
    {   // a bound of 0 on an own ring: internal
        Built b = voices_plan(7);
        b.sp.instrs[2].imm = 0;
        const StreamPlan s = b.plan();
        CHECK(!s.servable && s.reason.find("internal: ") == 0);
    }
    {   // the tiles: a sweep program is counted as a loop program
        Built b = voiceless_plan(7);
        std::vector<StageInstr> p = flanger(NO_RING, 0, 1, 7, 14, true);
        for (uint32_t k = 0; k < STREAM_LOOP_LOADS - 1; ++k) p.insert(p.begin(), ins(S_READ, 7, 0, 0, 0, 0, 100 + k));
        b.sp.instrs.clear(); b.sp.progs.clear();
        b.program(p, 0, NO_RING, 0);
        const StreamPlan s = b.plan();
        CHECK(!s.servable && s.reason == "a loop program has 33 frame-only loads; block streaming serves at most 32");
    }
    // (b) a signal tap behind a loop, in a feedback plan
    auto tap = [](uint32_t ring, uint32_t ring2) {
        std::vector<StageInstr> p{ins(S_INPUT, 3, 0, 0, 0, 0, 0), ins(S_READ_DYN, 0, 3, 0, 0, ring, 3)};
        if (ring2 != NO_RING) {
            p.push_back(ins(S_READ_DYN, 1, 3, 0, 0, ring2, 3));
            p.push_back(ins(S_SUM2, 0, 0, 1, 0, 0, 0));
        }
        return p;
    };
    {
        Built b = voices_plan(7);
        b.env.n_slots = 3;
        b.program(tap(3, NO_RING), 0, NO_RING, 2);                     // behind voice 1's flanger: it follows voice 1
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.voice_first == (std::vector<uint32_t>{0, 1, 3, 3}) && s.progs == (std::vector<uint32_t>{0, 1, 2}));
        CHECK(s.sweep_width == (std::vector<uint32_t>{7, 7, 0}) && s.loop_stride == (std::vector<uint32_t>{7, 7, 0}) && s.min_ring_delay == 0);
        CHECK(s.dyn_reads == 3 && s.dyn_ring_reads == 3 && s.short_reads == 3 && s.lookback == 14);
        CHECK(stream_launch(b.sp, s).kernel == StreamKernel::sweep);
        b.env.sweep = false;
        CHECK(b.plan().reason == OLD_SWEEP);
    }
    {   // a second one: the mix-bus sentence, or a bus program
        Built b = voices_plan(7);
        b.env.n_slots = 3;
        b.program(tap(2, 3), 0, NO_RING, 2);
        const StreamPlan s = b.plan();
        CHECK(!s.servable && s.reason == "a program reads voices 0 and 1 in the same block (a mix bus across voices); each streamed program follows one voice");
        b.env.bus = true;
        const StreamPlan t = b.plan();
        CHECK(t.servable && t.bus_programs() == 1 && t.voice_first == (std::vector<uint32_t>{0, 1, 2, 3}) && t.dyn_reads == 4 && t.short_reads == 4);
    }
    {   // a storer that comes LATER keeps today's sentence
        Built b;
        b.env = voices_plan(7).env;
        b.env.n_slots = 3;
        b.bank(7, true, {0, 1});
        b.sp.feedback = true;
        b.sp.fused_sweep = 7;
        b.sp.n_rings = 4;
        b.sp.input_slots = {0};
        b.program(tap(3, NO_RING), 0, NO_RING, 2);
        b.program(flanger(0, 2, 0, 7, 14, true), 0, NO_RING, 0);
        b.program(flanger(1, 3, 0, 7, 14, true), 0, NO_RING, 1);
        const StreamPlan s = b.plan();
        CHECK(!s.servable && s.reason == OLD_DYN_RING);
    }
    // (c) _DYN ops inside a loop program of constant stride (no sweep plan: fused_sweep == 0)
    auto chorus_comb = [](uint8_t dyn_op) {
        Built b;
        b.env.n_slots = 2;
        b.env.loops = b.env.dyn = b.env.sweep = true;
        b.bank(7, true, {0, 1});
        b.sp.feedback = true;
        b.sp.n_rings = 3;
        b.sp.input_slots = {0};
        std::vector<StageInstr> p = comb(0, 2, 8);
        p.insert(p.begin() + 1, {ins(S_INPUT, 3, 0, 0, 0, 0, 0), dyn_op == S_READ_DYN ? ins(S_READ_DYN, 0, 3, 0, 0, 0, 4) : dyn_op == S_STEP_DYN ? ins(S_STEP_DYN, 0, 3, 0, f32(1.0f), 0, 4)
                                                                                                                  : ins(S_READ_INPUT_DYN, 0, 3, 0, 0, 4, 0xFFFFFFFFu)});
        b.program(p, 0, NO_RING, 0);
        b.program(follow(1), 0, NO_RING, 1);
        return b;
    };
    {
        Built b = chorus_comb(S_READ_DYN);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.loop_stride == (std::vector<uint32_t>{8, 0}) && s.sweep_width == (std::vector<uint32_t>{0, 0}) && s.sweep_loops && s.has_sweep());
        CHECK(s.dyn_reads == 1 && s.dyn_ring_reads == 0 && s.min_ring_delay == 8);
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(l.kernel == StreamKernel::sweep && l.max_stride == 8 && l.max_loads == 3 && l.max_stores == 1);
        b.env.sweep = false;
        CHECK(!b.plan().servable && b.plan().reason == OLD_LOOP_DYN);
        Built c = chorus_comb(S_STEP_DYN);
        CHECK(c.plan().servable && c.plan().sweep_loops && c.plan().dyn_steps == 1);
        c.env.sweep = false;
        CHECK(c.plan().reason.find("a loop program uses S_STEP_DYN (a Delay by a signal amount inside a feedback loop shorter than a block)") == 0);
        Built h = chorus_comb(S_READ_INPUT_DYN);                       // without a history: today's sentence; with one it is served
        CHECK(!h.plan().servable && h.plan().reason.find("a program uses S_READ_INPUT_DYN (a delayed read of an input row)") == 0);
        h.env.history = true;
        const StreamPlan hs = h.plan();
        CHECK(hs.servable && hs.sweep_loops && hs.hist_dyn_reads == 1 && hs.input_lookback == 4 && stream_launch(h.sp, hs).kernel == StreamKernel::sweep &&
              stream_launch(h.sp, hs).hist_cap == 128);
        h.env.sweep = false;
        CHECK(h.plan().reason.find("a loop program uses S_READ_INPUT_DYN") == 0);
    }
    {   // a constant loop without a _DYN op keeps its kernel with the option on
        Built b = kernel_plan(StreamKernel::loops);
        b.env.dyn = b.env.sweep = true;
        const StreamPlan s = b.plan();
        CHECK(s.servable && !s.has_sweep() && s.sweep_width == (std::vector<uint32_t>{0, 0}) && stream_launch(b.sp, s).kernel == StreamKernel::loops);
    }
}

// ---- the form and the launch check of the four kernels ------------------------------------------------------------------------
static float2 some_params[1];
static float some_floats[1];
static uint32_t some_words[4];
static StageInstr some_instrs[1];
static StageProg some_progs[1];
static BankStreamInCtl some_ctl;
static BankStreamInDev some_dev;

static StreamLaunchArgs minimal(StreamKernel k) {
    const StreamForm f = stream_form(k);
    StreamLaunchArgs x{};
    x.a.params = some_params;
    x.a.out = some_floats;
    x.a.n_voices = f.voiceless ? 3 : 2;
    x.a.leaf_variant = 1;
    x.a.ws = some_floats;
    x.a.tickets = some_words;
    x.p.instrs = some_instrs;
    x.p.progs = some_progs;
    x.p.voice_first = some_words;
    x.p.rings = some_floats;
    x.p.ring_mask = 63;
    x.p.n_rings = 1;
    x.t.n_banks = 2;
    x.t.bank[0] = {some_params, some_words, 0, 0, 1, 7, 7, 1, 1};
    x.t.bank[1] = {some_params, some_words, 1, 1, 1, 9, 7, 1, 0};
    x.h.hist = some_floats;
    x.h.mask = 63;
    x.n_rows = 2;
    x.max_stride = 7; x.max_loads = 2; x.max_stores = 1;
    x.ctl_dev = &some_ctl;
    x.dev = &some_dev;
    return x;
}

static void test_form_and_check() {
    const struct { StreamKernel k, under; const char *name; } four[] = {
        {StreamKernel::sweep, StreamKernel::hist, "bank_stream_sweep_kernel"},
        {StreamKernel::sweep_fx, StreamKernel::fx, "bank_stream_sweep_fx_kernel"},
        {StreamKernel::sweep_store, StreamKernel::store, "bank_stream_sweep_store_kernel"},
        {StreamKernel::sweep_store_fx, StreamKernel::store_fx, "bank_stream_sweep_store_fx_kernel"}};
    CHECK((uint32_t)StreamKernel::sweep == (uint32_t)StreamKernel::store_fx + 2 && (uint32_t)StreamKernel::sweep_fx == (uint32_t)StreamKernel::sweep + 2 &&
          (uint32_t)StreamKernel::sweep_store == (uint32_t)StreamKernel::sweep_fx + 2 && (uint32_t)StreamKernel::sweep_store_fx == (uint32_t)StreamKernel::sweep_store + 2);
    const std::vector<std::pair<const char *, std::function<void(StreamLaunchArgs &)>>> breaks_all = {
        {"leaf_variant 0", [](StreamLaunchArgs &x) { x.a.leaf_variant = 0; }},
        {"out null", [](StreamLaunchArgs &x) { x.a.out = nullptr; }},
        {"ctl null", [](StreamLaunchArgs &x) { x.ctl_dev = nullptr; }},
        {"dev null", [](StreamLaunchArgs &x) { x.dev = nullptr; }},
        {"n_rows 0", [](StreamLaunchArgs &x) { x.n_rows = 0; }},
        {"n_rows 9", [](StreamLaunchArgs &x) { x.n_rows = BANK_STREAM_ROWS + 1; }},
        {"hist null", [](StreamLaunchArgs &x) { x.h.hist = nullptr; }},
        {"hist mask 62", [](StreamLaunchArgs &x) { x.h.mask = 62; }},
        {"hist of 32 frames", [](StreamLaunchArgs &x) { x.h.mask = 31; }},
        {"max_stride 64", [](StreamLaunchArgs &x) { x.max_stride = BANK_STREAM_LOOP_MAX_STRIDE + 1; }},
        {"max_loads 33", [](StreamLaunchArgs &x) { x.max_loads = BANK_STREAM_LOOP_LOADS + 1; }},
        {"max_stores 17", [](StreamLaunchArgs &x) { x.max_stores = BANK_STREAM_LOOP_STORES + 1; }},
        {"a loop, no rings", [](StreamLaunchArgs &x) { x.t.bank[0].to_ring = 0; x.p.n_rings = 0; }},
        {"no voices", [](StreamLaunchArgs &x) { x.a.n_voices = 0; }},
        {"257 workgroups", [](StreamLaunchArgs &x) { x.a.n_voices = 257; }},
        {"voice_first null", [](StreamLaunchArgs &x) { x.p.voice_first = nullptr; }},
        {"ring_mask 62", [](StreamLaunchArgs &x) { x.p.ring_mask = 62; }},
        {"rings null", [](StreamLaunchArgs &x) { x.p.rings = nullptr; }},
        {"rings of 32 frames", [](StreamLaunchArgs &x) { x.p.ring_mask = 31; }}};
    const std::vector<std::pair<const char *, std::function<void(StreamLaunchArgs &)>>> breaks_table = {
        {"n_banks 0", [](StreamLaunchArgs &x) { x.t.n_banks = 0; }},
        {"n_banks 9", [](StreamLaunchArgs &x) { x.t.n_banks = BANK_STREAM_BANKS + 1; }},
        {"bank chunk_log2 6", [](StreamLaunchArgs &x) { x.t.bank[1].chunk_log2 = 6; }},
        {"bank params null", [](StreamLaunchArgs &x) { x.t.bank[1].params = nullptr; }},
        {"bank rows null", [](StreamLaunchArgs &x) { x.t.bank[1].rows = nullptr; }},
        {"first_wg leaves a gap", [](StreamLaunchArgs &x) { x.t.bank[1].first_wg = 2; }},
        {"first_voice leaves a gap", [](StreamLaunchArgs &x) { x.t.bank[1].first_voice = 2; }},
        {"chunks without ws", [](StreamLaunchArgs &x) { x.a.ws = nullptr; }},
        {"chunks without tickets", [](StreamLaunchArgs &x) { x.a.tickets = nullptr; }},
        {"a bank feeds rings, no rings", [](StreamLaunchArgs &x) { x.p.n_rings = 0; x.max_stride = 0; }},
        {"mask beyond the table", [](StreamLaunchArgs &x) { x.g.mask = 1u << 2; }},
        {"a schedule bank without its schedule", [](StreamLaunchArgs &x) { x.g.mask = 1u << 1; }}};
    for (const auto &c : four) {
        const StreamForm f = stream_form(c.k), u = stream_form(c.under);
        CHECK(stream_kernel_named(c.k) && std::string(stream_kernel_name(c.k)) == c.name && stream_kernel_by_plan(c.k));
        CHECK(f.sweep && !u.sweep);
        CHECK(f.progs == u.progs && f.bus == u.bus && f.rows == u.rows && f.table == u.table && f.loops == u.loops && f.schedule == u.schedule && f.dyn == u.dyn &&
              f.hist == u.hist && f.voiceless == u.voiceless && f.store == u.store);
        CHECK(f.loops && f.dyn && f.hist && f.rows);
        const uint32_t wgs = f.voiceless ? 3u : 5u;
        CHECK(stream_launch_check(c.k, minimal(c.k)) == wgs && stream_launch_check(c.under, minimal(c.k)) == wgs);
        for (const auto &b : breaks_all) {
            StreamLaunchArgs x = minimal(c.k);
            b.second(x);
            if (stream_launch_check(c.k, x) != 0) { ++failed; std::printf("FAILED %s, %s: accepted\n", c.name, b.first); } else ++passed;
        }
        for (const auto &b : breaks_table) {                           // (the voiceless forms read neither the table nor ws and tickets)
            StreamLaunchArgs x = minimal(c.k);
            b.second(x);
            const uint32_t want = f.voiceless ? wgs : 0u;
            if (stream_launch_check(c.k, x) != want) { ++failed; std::printf("FAILED %s, %s: expected %u workgroups\n", c.name, b.first, want); } else ++passed;
        }
        StreamLaunchArgs x = minimal(c.k);                             // the accepted edges
        x.max_stride = BANK_STREAM_LOOP_MAX_STRIDE; x.max_loads = BANK_STREAM_LOOP_LOADS; x.max_stores = BANK_STREAM_LOOP_STORES; x.n_rows = BANK_STREAM_ROWS;
        CHECK(stream_launch_check(c.k, x) == wgs);
        for (uint32_t gap : {1u, 0xFFFFFFFFu})                         // the values in between stay unnamed and refused
        {
            const StreamKernel g = (StreamKernel)((uint32_t)c.k + gap);
            CHECK(!stream_kernel_named(g) && std::string(stream_kernel_name(g)) == "" && stream_launch_check(g, minimal(c.k)) == 0);
        }
    }
    CHECK(!stream_kernel_named((StreamKernel)((uint32_t)StreamKernel::sweep_store_fx + 2)) && !stream_kernel_named((StreamKernel)((uint32_t)StreamKernel::store_fx + 1)));
    for (StreamKernel k : {StreamKernel::plain, StreamKernel::prog, StreamKernel::loops, StreamKernel::dyn, StreamKernel::hist, StreamKernel::fx, StreamKernel::store,
                           StreamKernel::store_fx})
        CHECK(!stream_form(k).sweep);
}

// ---- the sweep walk against the sequential loop -------------------------------------------------------------------------------
constexpr uint32_t CAP = 256, MASK = CAP - 1, N_RINGS = 4, N_ROWS = 3;

static bool delay_frames(float d, uint64_t &frames, bool sparkle) {   // the reference's cast (kernels.hip delay_frames)
    if (d >= 18446744073709551616.0f) return false;
    if (sparkle && !(d >= 0.0f)) return false;
    frames = (d < 0.0f || d != d) ? 0ull : (uint64_t)d;
    return true;
}
static float binop(uint8_t op, float a, float b) {
    switch (op) {
    case S_SUM2: return a + b;
    case S_MUL: return a * b;
    case S_DIV: return a / b;
    case S_MOD: return std::fmod(a, b);
    default: return a < b ? a : b;
    }
}

// frame by frame, the plan's instructions as they are (stage_kernel's meaning of them)
static void evaluate(const StageProg &pg, const std::vector<StageInstr> &p, std::vector<float> &rings, const float (*rows)[64], uint64_t head, uint32_t n, float *out) {
    for (uint32_t f = 0; f < n; ++f) {
        const uint64_t t = head + f;
        float reg[STAGE_REGS] = {};
        for (const StageInstr &in : p) {
            uint64_t fr = 0;
            switch (in.op) {
            case S_CONST: reg[in.dst] = bitsf(in.imm); break;
            case S_INPUT: reg[in.dst] = rows[in.imm][f]; break;
            case S_READ: reg[in.dst] = t >= in.d_lo ? rings[in.buf * CAP + ((t - in.d_lo) & MASK)] : 0.0f; break;
            case S_STEP: reg[in.dst] = t >= in.d_lo ? bitsf(in.imm) : 0.0f; break;
            case S_STORE: rings[in.buf * CAP + (t & MASK)] = reg[in.a]; break;
            case S_READ_DYN: reg[in.dst] = delay_frames(reg[in.a], fr, false) && t >= fr ? rings[in.buf * CAP + ((t - fr) & MASK)] : 0.0f; break;
            case S_STEP_DYN: reg[in.dst] = delay_frames(reg[in.a], fr, false) && t >= fr ? bitsf(in.imm) : 0.0f; break;
            default: reg[in.dst] = binop(in.op, reg[in.a], reg[in.b]); break;
            }
        }
        if (pg.dst_ring != NO_RING) rings[pg.dst_ring * CAP + (t & MASK)] = reg[pg.result_reg];
        out[f] = reg[pg.result_reg];
    }
}

// the kernel's phases as plain loops over the 64 lanes, on the helper's output: phase 1 and 3 as the loops kernel's, phase 2 the walk
static void model(const StageProg &pg, const std::vector<StageInstr> &p, std::vector<float> &rings, const float (*rows)[64], uint64_t head, uint32_t n, float *out) {
    constexpr uint32_t LM = STREAM_LOOP_LOADS - 1, SM = STREAM_LOOP_STORES - 1;
    static float regs[STAGE_REGS][64], ldt[STREAM_LOOP_LOADS][64], stt[STREAM_LOOP_STORES][64];
    const uint32_t w = pg.pad[0] ? pg.pad[0] : 1;
    for (uint32_t lane = 0; lane < 64; ++lane) {                    // 1. lane = frame; a _DYN op takes no slot
        const uint64_t t = head + lane;
        uint32_t k = 0;
        for (const StageInstr &in : p) {
            if (in.op != S_INPUT && in.op != S_READ) continue;
            float v = 0.0f;
            const bool inside = in.op == S_READ && in.imm != 0 && lane >= in.d_lo;
            if (lane < n && !inside) v = in.op == S_INPUT ? rows[in.imm][lane] : t >= in.d_lo ? rings[in.buf * CAP + ((t - in.d_lo) & MASK)] : 0.0f;
            ldt[k++ & LM][lane] = v;
        }
    }
    for (uint32_t base = 0; base < n; base += w)                    // 2. the sweeps; the lanes of one sweep in the LEAST favourable order
        for (uint32_t lane = w; lane-- > 0;) {
            const uint32_t f = base + lane;
            if (f >= n) continue;
            uint32_t k = 0;
            for (const StageInstr &in : p) {
                float v;
                uint64_t fr = 0;
                switch (in.op) {
                case S_CONST: v = bitsf(in.imm); break;
                case S_STEP: v = head + f >= in.d_lo ? bitsf(in.imm) : 0.0f; break;
                case S_INPUT: v = ldt[k++ & LM][f]; break;
                case S_READ: {
                    const uint32_t slot = k++ & LM;
                    v = in.imm != 0 && f >= in.d_lo ? stt[(in.imm - 1) & SM][(f - in.d_lo) & 63] : ldt[slot][f];
                    break;
                }
                case S_STORE: stt[(in.imm - 1) & SM][f] = regs[in.a][f]; continue;
                case S_READ_DYN:
                    if (!delay_frames(regs[in.a][f], fr, false) || head + f < fr) v = 0.0f;
                    else if (in.imm != 0 && fr <= f) v = stt[(in.imm - 1) & SM][(f - (uint32_t)fr) & 63];
                    else v = rings[in.buf * CAP + ((head + f - fr) & MASK)];
                    break;
                case S_STEP_DYN: v = delay_frames(regs[in.a][f], fr, false) && head + f >= fr ? bitsf(in.imm) : 0.0f; break;
                default: v = binop(in.op, regs[in.a][f], regs[in.b][f]); break;
                }
                regs[in.dst][f] = v;
            }
        }
    for (uint32_t lane = 0; lane < n; ++lane) {                     // 3. the live lanes store
        for (const StageInstr &in : p)
            if (in.op == S_STORE) rings[in.buf * CAP + ((head + lane) & MASK)] = stt[(in.imm - 1) & SM][lane];
        out[lane] = regs[pg.result_reg][lane];
    }
}

// A random sweep program of width w over ring 0 (a voice's, filled by the test), rings 1..own (its own) and ring 3 (an earlier
// program's, filled by the test).  The amounts are input rows: row 1 holds values in [w, w + span], row 2 values in [0, 40] (for
// the rings that are not its own, and for S_STEP_DYN).
static std::vector<StageInstr> random_program(std::mt19937 &rng, uint32_t own, uint32_t w, StageProg &pg) {
    auto pick = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    const float gains[] = {0.25f, -0.25f, 0.3f, -0.125f, 0.125f};
    std::vector<StageInstr> p{ins(S_INPUT, 10, 0, 0, 1, 0, 0), ins(S_INPUT, 11, 0, 0, 2, 0, 0)};
    uint32_t last = 0;
    for (uint32_t part = 0; part < own; ++part) {
        const uint8_t acc = 0, tmp = 1, c = 2;
        switch (pick(3)) {
        case 0: p.push_back(ins(S_READ, acc, 0, 0, pick(200), 0, 0)); break;
        case 1: p.push_back(ins(S_INPUT, acc, 0, 0, 0, 0, 0)); break;
        default: p.push_back(ins(S_READ_DYN, acc, 11, 0, 0, pick(2) ? 0 : 3, 40)); break;   // a voice or an earlier program, 0 frames included
        }
        // the first read of the first part is the own-ring S_READ_DYN with the bound w; the others anything at least w frames back
        const uint32_t reads = 1 + pick(3);
        for (uint32_t r = 0; r < reads; ++r) {
            const uint32_t ring = 1 + pick(own);
            if ((part == 0 && r == 0) || pick(2)) p.push_back(ins(S_READ_DYN, tmp, 10, 0, w, ring, w + 70));
            else p.push_back(ins(S_READ, tmp, 0, 0, pick(256), ring, w + pick(100)));
            p.push_back(ins(S_CONST, c, 0, 0, f32(gains[pick(5)]), 0, 0));
            p.push_back(ins(S_MUL, tmp, tmp, c, 0, 0, 0));
            p.push_back(ins(pick(8) ? S_SUM2 : S_MIN, acc, acc, tmp, 0, 0, 0));
        }
        if (pick(3) == 0) {
            p.push_back(pick(2) ? ins(S_STEP, tmp, 0, 0, f32(0.0625f), 0, 30 + pick(300)) : ins(S_STEP_DYN, tmp, 11, 0, f32(0.0625f), 0, 40));
            p.push_back(ins(S_SUM2, acc, acc, tmp, 0, 0, 0));
        }
        last = 1 + part;
        if (part + 1 < own || pick(2)) { p.push_back(ins(S_STORE, 0, acc, 0, pick(9), last, 0)); last = 0; }
    }
    pg = prog(p, 0, last ? last : NO_RING, 0);
    return p;
}

static void test_walk() {
    std::mt19937 rng(20261020);
    for (int trial = 0; trial < 60; ++trial) {
        const uint32_t widths[] = {1, 7, 63};
        const uint32_t w = widths[trial % 3], own = 1 + (trial / 3) % 2;
        StageProg pg;
        const std::vector<StageInstr> p = random_program(rng, own, w, pg);
        StageProg spg = pg;
        std::vector<StageInstr> sp = p;
        CHECK(stream_sweep_prepare(spg, sp));
        CHECK(spg.pad[0] == w && stream_sweep_width(pg, p.data()) == w);
        std::vector<float> ra(N_RINGS * CAP, 0.0f), rb(N_RINGS * CAP, 0.0f);
        uint64_t head = trial % 4 == 0 ? 0 : rng() % 1000;
        bool same = true, short_block = false;
        const uint32_t span = trial % 2 ? 64 : 3;                       // amounts that stay near the bound, amounts that leave the block
        for (int block = 0; block < 300 && same; ++block) {
            const uint32_t n = block % 7 == 3 ? 1 + rng() % 6 : 1 + rng() % 64;
            short_block = short_block || n < w;
            float rows[N_ROWS][64];
            for (uint32_t f = 0; f < 64; ++f) {
                rows[0][f] = (float)((int)(rng() % 2001) - 1000) / 512.0f;
                rows[1][f] = (float)w + (float)(rng() % (span * 4 + 1)) / 4.0f;     // in [w, w + span], quarters: the cast floors
                rows[2][f] = (float)(rng() % 161) / 4.0f;                          // in [0, 40]
            }
            for (uint32_t f = 0; f < n; ++f)                        // the voice's frames and the earlier program's, stored before this one runs
                for (uint32_t ring : {0u, 3u}) ra[ring * CAP + ((head + f) & MASK)] = rb[ring * CAP + ((head + f) & MASK)] = (float)((int)(rng() % 4001) - 2000) / 1024.0f;
            float oa[64] = {}, ob[64] = {};
            evaluate(pg, p, ra, rows, head, n, oa);
            model(spg, sp, rb, rows, head, n, ob);
            same = std::memcmp(oa, ob, n * sizeof(float)) == 0 && std::memcmp(ra.data(), rb.data(), ra.size() * sizeof(float)) == 0;
            head += n;
        }
        CHECK(same);
        CHECK(head > CAP);                                          // the rings wrapped
        CHECK(w == 1 || short_block);                               // a block shorter than a sweep was among them
    }
}

int main() {
    test_helpers();
    test_rule();
    test_form_and_check();
    test_walk();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
