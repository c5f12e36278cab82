// streamhist_tests.cpp -- FR_STREAM_HISTORY on the host (libfriendship_amd/csrc/streamplan.hpp, kernels.hpp): the serving rule on
// hand-built plans (a delayed read of an input row in a voice's program, a bus program and a loop program; its slot; a signal
// amount with and without FR_STREAM_DYN, with and without a proven bound, inside a loop, next to an observed bound; the
// look-back and its limit; the option off), the launch rule (hist on top of the cascade and for those plans alone, the
// history's capacity, the schedule table only with schedule banks, the kernel's number and name), stream_launch_check of the
// hist form with every checked field broken one at a time, and a plain-loop model of the history at capacity -- blocks of
// random length stored as wave 0 of workgroup 0 stores them, then read as kernels.hip's StreamHistInput and stream_prog_dyn
// read them -- against a model that keeps every sample.  Stand-alone: built and run on the CPU with -fsanitize=address,undefined
// by tests/test_stream_hist_host.py.
#include <cmath>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "streamplans.hpp"

static bool has(const std::string &s, const char *w) { return s.find(w) != std::string::npos; }

// voice ring * Delay(In(input), d)
static std::vector<StageInstr> gate(uint32_t voice_ring, uint32_t input, uint32_t d) {
    return {ins(S_READ, 0, 0, 0, 0, voice_ring, 0), ins(S_READ_INPUT, 1, 0, 0, input, 0, d), ins(S_MUL, 0, 0, 1, 0, 0, 0)};
}
// voice ring + Delay(In(input), amount in r1 = In(0)); `bound` as the planner leaves it in buf, d_lo says "unbounded"
static std::vector<StageInstr> dyn_gate(uint32_t voice_ring, uint32_t input, uint32_t bound) {
    return {ins(S_READ, 0, 0, 0, 0, voice_ring, 0), ins(S_INPUT, 1, 0, 0, 0, 0, 0), ins(S_READ_INPUT_DYN, 2, 1, 0, input, bound, 0xFFFFFFFFu), ins(S_SUM2, 0, 0, 2, 0, 0, 0)};
}

// two voices of 128 partials behind rings 0 and 1, row v = voice v * Delay(In(slot 3), d)
static Built two_gates(uint32_t d) {
    Built b;
    b.env.n_slots = 2;
    b.env.history = b.env.inputs = true;
    b.bank(7, true, {0, 1});
    b.sp.n_rings = 2;
    b.sp.input_slots = {0, 3};
    b.program(gate(0, 1, d), 0, NO_RING, 0);
    b.program(gate(1, 1, d), 0, NO_RING, 1);
    return b;
}

static const char *const OLD = "a program uses S_READ_INPUT (a delayed read of the input row), which block streaming does not serve yet";
static const char *const OLD_DYN = "a program uses S_READ_INPUT (a delayed read of an input row), which block streaming does not serve yet: a stream keeps no input history";

static void test_rule() {
    for (uint32_t d : {0u, 1u, 63u, 64u, 65u, 100u, 1u << 20}) {       // any constant delay, below a block included
        Built b = two_gates(d);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.reason.empty() && s.has_hist() && s.hist_reads == 2 && s.hist_dyn_reads == 0 && s.input_lookback == d);
        CHECK(s.programs_per_voice() == (std::vector<uint32_t>{1, 1}) && s.bus_programs() == 0 && s.input_slots == (std::vector<uint32_t>{0, 3}));
        CHECK(s.lookback == 0 && !s.has_dyn());                          // (the rings' look-back is another matter)
        b.env.bus = true;                                                // it reads no voice: never a bus program
        CHECK(b.plan().servable && b.plan().bus_programs() == 0);
        b.env.history = false;                                           // without the option: today's texts, word for word
        const StreamPlan off = b.plan();
        CHECK(!off.servable && off.reason == OLD && !off.has_hist() && off.input_lookback == 0);
        b.env.dyn = true;
        CHECK(b.plan().reason == OLD_DYN);
    }
    {   // the look-back over the limit: refused with the value and the limit
        Built b = two_gates((1u << 20) + 1);
        const StreamPlan s = b.plan();
        CHECK(!s.servable && has(s.reason, "reads an input row 1048577 frames back") && has(s.reason, "holds at most 1048576 frames"));
        CHECK(stream_hist_cap(1u << 20) == 1u << 21 && STREAM_HIST_MAX_FRAMES == 1u << 20);
    }
    {   // the slot: another one than 0 needs FR_STREAM_INPUTS, with that refusal's text; slot 0 delayed needs nothing more
        Built b = two_gates(7);
        b.env.inputs = false;
        CHECK(!b.plan().servable && b.plan().reason == "a program reads input slot 3; block streaming feeds slot 0 only");
        b.sp.instrs[1].imm = b.sp.instrs[4].imm = 0;                     // Delay(In(0), 7): the time row itself
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.input_slots == (std::vector<uint32_t>{0}) && s.hist_reads == 2 && s.input_lookback == 7);
        CHECK(stream_launch(b.sp, s).kernel == StreamKernel::hist && stream_launch(b.sp, s).n_rows == 1);
        b.sp.instrs[1].imm = 9;                                          // an input index the plan does not have
        CHECK(!b.plan().servable && has(b.plan().reason, "a program reads input slot 9"));
    }
    {   // nine distinct slots, delayed or not: the limit's own text
        Built b = two_gates(7);
        b.sp.input_slots = {0, 1, 2, 3, 4, 5, 6, 7, 8};
        std::vector<StageInstr> p{ins(S_READ, 0, 0, 0, 0, 0, 0)};
        for (uint32_t k = 1; k < 9; ++k) p.push_back(ins(k & 1 ? S_READ_INPUT : S_INPUT, 1, 0, 0, k, 0, k & 1 ? 10 * k : 0));
        b.sp.instrs.clear(); b.sp.progs.clear();
        b.program(p, 0, NO_RING, 0);
        b.program(follow(1), 0, NO_RING, 1);
        CHECK(!b.plan().servable && has(b.plan().reason, "9 distinct input slots (slot 0 included); block streaming feeds at most 8"));
        b.sp.instrs[8] = ins(S_READ_INPUT, 1, 0, 0, 7, 0, 80);           // slot 7 twice: eight slots
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.input_slots.size() == 8 && s.hist_reads == 5 && s.input_lookback == 80);
    }
    {   // a bus program (FR_STREAM_BUS) may hold one; the per-voice program next to it stays its voice's
        Built b = two_gates(30);
        b.env.bus = true;
        b.env.n_slots = 3;
        b.program({ins(S_READ, 0, 0, 0, 0, 0, 0), ins(S_READ, 1, 0, 0, 0, 1, 0), ins(S_SUM2, 0, 0, 1, 0, 0, 0), ins(S_READ_INPUT, 1, 0, 0, 1, 0, 70), ins(S_MUL, 0, 0, 1, 0, 0, 0)},
                  0, NO_RING, 2);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.bus_programs() == 1 && s.programs_per_voice() == (std::vector<uint32_t>{1, 1}) && s.hist_reads == 3 && s.input_lookback == 70);
    }
    {   // a signal amount: with FR_STREAM_DYN and a proven bound (buf), whatever the bound; the look-back is the bound
        for (uint32_t bound : {0u, 31u, 48u, 700u}) {
            Built b = two_gates(5);
            b.env.dyn = true;
            b.sp.instrs.clear(); b.sp.progs.clear();
            b.program(dyn_gate(0, 1, bound), 0, NO_RING, 0);
            b.program(gate(1, 1, 5), 0, NO_RING, 1);
            const StreamPlan s = b.plan();
            CHECK(s.servable && s.hist_dyn_reads == 1 && s.hist_reads == 1 && s.input_lookback == std::max(bound, 5u) && !s.has_dyn());
            CHECK(stream_launch(b.sp, s).kernel == StreamKernel::hist);
            b.env.dyn = false;                                           // without it: a Delay by a signal amount, today's text
            CHECK(b.plan().reason == "a program uses S_READ_INPUT_DYN (a Delay by a signal amount), which block streaming does not serve yet");
            b.env.dyn = true;
            b.env.history = false;
            CHECK(has(b.plan().reason, "S_READ_INPUT_DYN (a delayed read of an input row)") && has(b.plan().reason, "a stream keeps no input history"));
            b.env.history = true;
            b.sp.observed.push_back({1u, 512u});                         // a bound observed from input rows stays refused
            CHECK(!b.plan().servable && has(b.plan().reason, "a Delay's bound was observed from input rows (FR_DELAY_OBSERVED)"));
        }
        Built b = two_gates(5);                                          // no proven bound: the history is finite
        b.env.dyn = true;
        b.sp.instrs.clear(); b.sp.progs.clear();
        b.program(dyn_gate(0, 1, 0xFFFFFFFFu), 0, NO_RING, 0);
        b.program(follow(1), 0, NO_RING, 1);
        CHECK(!b.plan().servable && has(b.plan().reason, "by a signal amount without a proven bound"));
    }
    {   // inside a loop program (FR_STREAM_LOOPS): one more frame-only load; a signal amount there stays refused
        Built b;
        b.env.n_slots = 2;
        b.env.history = b.env.inputs = b.env.loops = true;
        b.bank(7, true, {0, 1});
        b.sp.feedback = true;
        b.sp.n_rings = 3;
        b.sp.input_slots = {0, 1};
        std::vector<StageInstr> loop = comb(0, 2, 5);
        loop.insert(loop.begin() + 2, {ins(S_READ_INPUT, 2, 0, 0, 1, 0, 3), ins(S_SUM2, 0, 0, 2, 0, 0, 0)});
        b.program(loop, 0, NO_RING, 0);
        b.program(follow(1), 0, NO_RING, 1);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.loop_stride == (std::vector<uint32_t>{5, 0}) && s.hist_reads == 1 && s.input_lookback == 3 && s.min_ring_delay == 5);
        CHECK(stream_loop_loads(b.sp.progs[0], b.sp.instrs.data()) == 3);   // the voice's ring, the own read, the delayed input
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(l.kernel == StreamKernel::hist && l.max_stride == 5 && l.max_loads == 3 && l.max_stores == 1 && l.hist_cap == 128);
        StageProg pg = b.sp.progs[0];                                    // the stream's copy: the read keeps its operand (the engine rewrites it to the row)
        std::vector<StageInstr> own(b.sp.instrs.begin(), b.sp.instrs.begin() + pg.n_instr);
        CHECK(stream_loop_prepare(pg, own) && pg.pad[0] == 5 && own[2].op == S_READ_INPUT && own[2].imm == 1 && own[2].d_lo == 3);
        {   // the load limit counts it
            Built c = b;
            std::vector<StageInstr> many = comb(0, 2, 5);
            for (uint32_t k = 0; k < STREAM_LOOP_LOADS - 2; ++k) many.insert(many.begin() + 2, ins(S_READ_INPUT, 2, 0, 0, 1, 0, k));
            c.sp.instrs.clear(); c.sp.progs.clear();
            c.program(many, 0, NO_RING, 0);
            c.program(follow(1), 0, NO_RING, 1);
            CHECK(c.plan().servable && stream_launch(c.sp, c.plan()).max_loads == STREAM_LOOP_LOADS);
            many.insert(many.begin() + 2, ins(S_READ_INPUT, 2, 0, 0, 1, 0, 9));
            c.sp.instrs.clear(); c.sp.progs.clear();
            c.program(many, 0, NO_RING, 0);
            c.program(follow(1), 0, NO_RING, 1);
            CHECK(!c.plan().servable && has(c.plan().reason, "a loop program has 33 frame-only loads; block streaming serves at most 32"));
        }
        b.env.dyn = true;
        b.sp.instrs[2] = ins(S_READ_INPUT_DYN, 2, 0, 0, 1, 31, 0xFFFFFFFFu);
        CHECK(!b.plan().servable && has(b.plan().reason, "a loop program uses S_READ_INPUT_DYN") && has(b.plan().reason, "inside a feedback loop shorter than a block"));
        b.env.history = false;                                           // the option off: the loop's pre-check does not know the op
        CHECK(has(b.plan().reason, "S_READ_INPUT_DYN (a delayed read of an input row)"));
    }
}

// ---- the launch rule ---------------------------------------------------------------------------------------------------
static void test_launch() {
    CHECK((uint32_t)StreamKernel::hist == (uint32_t)StreamKernel::dyn + 2);
    CHECK(std::strcmp(stream_kernel_name(StreamKernel::hist), "bank_stream_hist_kernel") == 0 && stream_kernel_by_plan(StreamKernel::hist));
    CHECK(std::strcmp(stream_kernel_name((StreamKernel)((uint32_t)StreamKernel::dyn + 1)), "") == 0);
    CHECK(std::strcmp(stream_kernel_name((StreamKernel)((uint32_t)StreamKernel::hist + 1)), "") == 0);
    CHECK(stream_kernel_named(StreamKernel::hist) && stream_kernel_named(StreamKernel::dyn) && !stream_kernel_named((StreamKernel)((uint32_t)StreamKernel::dyn + 1)) &&
          !stream_kernel_named(StreamKernel::none) && !stream_kernel_named((StreamKernel)((uint32_t)StreamKernel::hist + 1)));
    constexpr StreamForm f = stream_form(StreamKernel::hist), d = stream_form(StreamKernel::dyn);
    static_assert(f.progs && f.bus && f.rows && f.table && f.loops && f.schedule && f.dyn && f.hist, "hist is dyn's form and the history");
    static_assert(d.dyn && !d.hist && !stream_form(StreamKernel::general).dyn && !stream_form(StreamKernel::general).hist, "");
    for (uint32_t look : {0u, 1u, 63u, 64u, 65u, 100u, 192u, 193u, 1u << 20}) {   // the power of two >= look-back + a block
        const uint64_t cap = stream_hist_cap(look);
        CHECK((cap & (cap - 1)) == 0 && cap >= (uint64_t)look + 64 && (cap == 64 || cap / 2 < (uint64_t)look + 64));
    }
    {   // one bank, two slots: rows doorbell, own instructions, bank table, no schedule table; the capacity from the look-back
        const Built b = two_gates(100);
        const StreamLaunch l = stream_launch(b.sp, b.plan());
        CHECK(l.kernel == StreamKernel::hist && l.rows_doorbell && l.n_rows == 2 && l.own_instrs && l.bank_table && !l.schedule_table && l.by_plan);
        CHECK(l.hist_cap == 256 && l.workgroups == 2 && l.max_stride == 0);
    }
    {   // with a schedule bank: the schedule table too; without the reads: the kernel below, no history
        Built b = two_gates(20);
        b.env.banks = b.env.general = true;
        b.env.n_slots = 3;
        b.bank(5, false, {2});
        const StreamPlan s = b.plan();
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(s.servable && s.has_general() && l.kernel == StreamKernel::hist && l.schedule_table && l.bank_table && l.hist_cap == 128 && l.workgroups == 3);
        for (StageInstr &i : b.sp.instrs)
            if (i.op == S_READ_INPUT) i = ins(S_INPUT, i.dst, 0, 0, i.imm, 0, 0);
        const StreamLaunch m = stream_launch(b.sp, b.plan());
        CHECK(b.plan().servable && !b.plan().has_hist() && m.kernel == StreamKernel::general && m.hist_cap == 0 && m.schedule_table && m.n_rows == l.n_rows);
    }
    for (StreamKernel k : {StreamKernel::prog, StreamKernel::bus, StreamKernel::in, StreamKernel::banks, StreamKernel::loops, StreamKernel::general, StreamKernel::dyn}) {
        Built b = kernel_plan(k);                                        // plans without a delayed input: the option changes nothing
        const StreamLaunch off = stream_launch(b.sp, b.plan());
        b.env.history = true;
        const StreamPlan s = b.plan();
        const StreamLaunch on = stream_launch(b.sp, s);
        CHECK(s.servable && !s.has_hist() && s.input_lookback == 0 && on.kernel == k && off.kernel == k && on.hist_cap == 0 && on.workgroups == off.workgroups &&
              on.n_rows == off.n_rows && on.schedule_table == off.schedule_table);
    }
}

// ---- stream_launch_check of the hist form ----------------------------------------------------------------------------------
static float2 some_params[1];
static float some_floats[1];
static uint32_t some_words[4];
static StageInstr some_instrs[1];
static StageProg some_progs[1];
static BankStreamInCtl some_ctl;
static BankStreamInDev some_dev;

static StreamLaunchArgs minimal() {   // (tests/cpp/streamcheck_tests.cpp's minimal arguments of a schedule form, and a history)
    StreamLaunchArgs x{};
    x.a.params = some_params; x.a.out = some_floats; x.a.rows = some_words;
    x.a.n_voices = 3; x.a.log2_p = x.a.chunk_log2 = 7; x.a.leaf_variant = 1; x.a.ws = some_floats; x.a.tickets = some_words;
    x.p.instrs = some_instrs; x.p.progs = some_progs; x.p.voice_first = some_words; x.p.rings = some_floats; x.p.ring_mask = 63; x.p.n_rings = 1;
    x.t.n_banks = 3;
    x.t.bank[0] = {some_params, some_words, 0, 0, 1, 7, 7, 1, 1};
    x.t.bank[1] = {some_params, some_words, 1, 1, 1, 9, 7, 1, 0};
    x.t.bank[2] = {some_params, some_words, 5, 2, 1, 0, 0, 1, 0};
    x.g.mask = 1u << 2;
    x.g.bank[2].groups = x.g.bank[2].group_off = some_words;
    x.h.hist = some_floats; x.h.mask = 255;
    x.n_rows = 2; x.max_stride = 5; x.max_loads = 3; x.max_stores = 1;
    x.ctl_dev = &some_ctl; x.dev = &some_dev;
    return x;
}

static void test_check() {
    const StreamKernel H = StreamKernel::hist;
    CHECK(stream_launch_check(H, minimal()) == 6);
    auto broken = [&](auto &&apply) { StreamLaunchArgs x = minimal(); apply(x); return stream_launch_check(H, x); };
    // the history's own fields
    CHECK(broken([](StreamLaunchArgs &x) { x.h.hist = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.h.mask = 254; }) == 0);                     // not 2^n - 1
    CHECK(broken([](StreamLaunchArgs &x) { x.h.mask = 100; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.h.mask = 31; }) == 0);                      // a capacity below a block
    CHECK(broken([](StreamLaunchArgs &x) { x.h.mask = 0; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.h.mask = ~0ull; }) == 0);                   // (mask + 1 wraps to 0)
    CHECK(broken([](StreamLaunchArgs &x) { x.h.mask = 63; }) == 6);                      // the smallest: one block
    CHECK(broken([](StreamLaunchArgs &x) { x.h.mask = (1ull << 21) - 1; }) == 6);
    // everything the dyn form checks, one at a time
    CHECK(broken([](StreamLaunchArgs &x) { x.a.leaf_variant = 0; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.a.out = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.ctl_dev = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.dev = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.n_rows = 0; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.n_rows = BANK_STREAM_ROWS + 1; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.n_rows = BANK_STREAM_ROWS; }) == 6);
    CHECK(broken([](StreamLaunchArgs &x) { x.max_stride = BANK_STREAM_LOOP_MAX_STRIDE + 1; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.max_loads = BANK_STREAM_LOOP_LOADS + 1; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.max_stores = BANK_STREAM_LOOP_STORES + 1; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.t.bank[0].to_ring = 0; x.p.n_rings = 0; }) == 0);   // a loop lives in a ring
    CHECK(broken([](StreamLaunchArgs &x) { x.t.n_banks = 0; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.t.n_banks = BANK_STREAM_BANKS + 1; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.t.bank[1].chunk_log2 = 6; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.t.bank[1].params = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.t.bank[1].rows = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.t.bank[1].first_wg = 2; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.t.bank[1].first_voice = 2; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.t.bank[0].n_voices = 257; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.a.n_voices = 4; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.a.ws = nullptr; }) == 0);                   // bank 1 has four chunks
    CHECK(broken([](StreamLaunchArgs &x) { x.a.tickets = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.g.mask |= 1u << 3; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.g.bank[2].groups = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.g.bank[2].group_off = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.p.voice_first = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.p.ring_mask = 62; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.p.rings = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.p.ring_mask = 31; }) == 0);
    // like dyn it takes a plan without a schedule bank (mask == 0), and one without rings or loops
    CHECK(broken([](StreamLaunchArgs &x) { x.g = StreamGeneralArgs{}; x.t.bank[2].log2_p = x.t.bank[2].chunk_log2 = 7; }) == 6);
    CHECK(broken([](StreamLaunchArgs &x) { x.t.bank[0].to_ring = 0; x.p.n_rings = 0; x.p.rings = nullptr; x.p.ring_mask = 0; x.max_stride = 0; }) == 6);
    // the other eight kernels read neither field
    for (StreamKernel k : {StreamKernel::plain, StreamKernel::prog, StreamKernel::bus, StreamKernel::in, StreamKernel::banks, StreamKernel::loops, StreamKernel::general,
                           StreamKernel::dyn}) {
        StreamLaunchArgs x = minimal();
        if (!stream_form(k).schedule) { x.a.n_voices = stream_form(k).table ? 2 : 1; x.t.n_banks = 2; x.p.bank_to_ring = 1; }
        const uint32_t with = stream_launch_check(k, x);
        x.h.hist = nullptr; x.h.mask = 12345;
        CHECK(with != 0 && stream_launch_check(k, x) == with);
    }
    // the value after dyn, and the one after hist: no kernel
    CHECK(stream_launch_check((StreamKernel)((uint32_t)StreamKernel::dyn + 1), minimal()) == 0);
    CHECK(stream_launch_check((StreamKernel)((uint32_t)StreamKernel::hist + 1), minimal()) == 0);
    CHECK(stream_launch_check(StreamKernel::none, minimal()) == 0 && stream_launch_check((StreamKernel)0xFFFFFFFFu, minimal()) == 0);
}

// ---- the history at capacity: the kernel's stores and loads as plain loops ----------------------------------------------------
// kernels.hip delay_frames (tests/cpp/streamdyn_tests.cpp has the cast's own checks)
static bool delay_frames(float d, uint64_t &frames, bool sparkle) {
    if (d >= 18446744073709551616.0f) return false;
    if (sparkle && !(d >= 0.0f)) return false;
    frames = (d < 0.0f || d != d) ? 0ull : (uint64_t)d;
    return true;
}
static uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

struct History {                      // `hist` has rows * (mask + 1) floats, exactly (ASan watches both ends)
    std::vector<float> hist;
    uint64_t mask;
    uint32_t rows;
    History(uint32_t rows_, uint64_t cap) : hist((size_t)rows_ * cap, 0.0f), mask(cap - 1), rows(rows_) {}   // zeroed: what a seek leaves
    // kernels.hip StreamHistoryStore: wave 0 of workgroup 0, lane < T
    void store(uint32_t row, uint64_t head, uint32_t T, const float *v) {
        for (uint32_t lane = 0; lane < 64; ++lane)
            if (lane < T) hist[(size_t)row * (mask + 1) + ((head + lane) & mask)] = v[lane];
    }
    // kernels.hip StreamHistInput::at behind stream_prog_load's range test
    float read(uint32_t row, uint64_t frame, uint32_t d) const { return frame >= d ? hist[(size_t)(row & 7u) * (mask + 1) + ((frame - d) & mask)] : 0.0f; }
    // kernels.hip stream_prog_dyn with the history as its rings
    float read_dyn(uint32_t row, uint64_t frame, float amount, bool sparkle) const {
        uint64_t fr;
        if (!delay_frames(amount, fr, sparkle) || frame < fr) return 0.0f;
        return hist[(size_t)(row & 7u) * (mask + 1) + ((frame - fr) & mask)];
    }
};

static void test_history() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    std::mt19937 rng(0x415);
    for (uint32_t look : {0u, 1u, 63u, 64u, 65u, 100u, 192u, 700u}) {
        for (uint64_t seek : {0ull, 69ull, 5003ull, (1ull << 32) - 100, 1ull << 62}) {   // the stream's first frame (a seek: zeros before it)
            const uint64_t cap = stream_hist_cap(look);
            const uint32_t rows = 3;
            History h(rows, cap);
            std::vector<std::vector<float>> all(rows);                                     // the model that keeps every sample, from `seek` on
            auto sample = [&](uint32_t row, uint64_t frame) { return frame < seek ? 0.0f : all[row][frame - seek]; };
            uint64_t head = seek;
            const float amounts[] = {-1.0f, -0.0f, 0.0f, 0.5f, 1.0f, 63.0f, 64.0f, 65.0f, (float)look, (float)look + 0.99f, nan, -inf};
            for (int block = 0; block < 40; ++block) {
                const uint32_t T = block < 2 ? 64 : 1 + rng() % 64;
                float v[64];
                for (uint32_t row = 0; row < rows; ++row) {
                    for (uint32_t i = 0; i < 64; ++i) v[i] = i < T ? (float)(row * 1000000u) + (float)((head + i) % 900001u) * 0.5f + 1.0f : nan;
                    for (uint32_t i = 0; i < T; ++i) all[row].push_back(v[i]);
                    h.store(row, head, T, v);
                }
                for (uint32_t row = 0; row < rows; ++row)
                    for (uint32_t lane = 0; lane < T; ++lane) {                            // live lanes, lane = frame
                        const uint64_t frame = head + lane;
                        for (uint32_t d : {0u, std::min(1u, look), look / 2, look}) {   // (within the look-back the capacity was made for)
                            const float want = frame >= d ? sample(row, frame - d) : 0.0f;
                            if (bits(h.read(row, frame, d)) != bits(want)) { ++failed; std::printf("FAILED look %u seek %llu frame %llu d %u\n", look, (unsigned long long)seek, (unsigned long long)frame, d); }
                            else ++passed;
                        }
                        for (bool sparkle : {false, true})
                            for (float amount : amounts) {
                                uint64_t fr = 0;
                                const bool cast = delay_frames(amount, fr, sparkle);
                                if (cast && fr > look) continue;                           // (beyond the proven bound: the planner's business)
                                const float want = !cast || frame < fr ? 0.0f : sample(row, frame - fr);
                                CHECK(bits(h.read_dyn(row, frame, amount, sparkle)) == bits(want));
                            }
                        // hostile amounts beyond the bound: an address inside the history all the same
                        for (float amount : {1e9f, 4294967296.0f, 9223372036854775808.0f, 18446744073709551616.0f, inf})
                            (void)h.read_dyn(row, frame, amount, false);
                    }
                head += T;
            }
        }
    }
}

int main() {
    test_rule();
    test_launch();
    test_check();
    test_history();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
