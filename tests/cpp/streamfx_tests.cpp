// streamfx_tests.cpp -- FR_STREAM_EFFECTS on the host (libfriendship_amd/csrc/streamplan.hpp, kernels.hpp): the serving rule on
// hand-built plans WITHOUT a bank launch (groups and segments, the wrap of the groups over four workgroups, a tap and a row copy
// that follow their loop's group, bus detection without any bank ring, every refusal with its text, the option off), the launch
// rule (fx exactly for a plan without a voice, its workgroups, a history of at least a block), the kernels' numbers, names and
// forms (the nine older ones unchanged), stream_launch_check of the fx form with every checked field broken one at a time, and
// a plain-loop model of ONE SEGMENT's block -- kernels.hip's interpreter and the three phases of a loop program, on the stream's
// own prepared instructions -- against a dense frame-by-frame recurrence for comb_5 and tap_behind of tests/stream_fx_cases.py.
// Stand-alone: built and run on the CPU with -fsanitize=address,undefined by tests/test_stream_fx_host.py.
#include <cmath>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "streamplans.hpp"

static const char *const OLD = "block streaming needs a plan with one voice bank (this one: 0 bank launches)";
static const char *const NO_FUSED = "the plan has no fused form: a program's ring is read less than 64 frames back (or the fused programs exceed the interpreter's budget)";
static const char *const DYN_OF_A_PROGRAM =
    "a program uses S_READ_DYN of a ring that a program stores (a Delay of a computed value by a signal amount, which may be 0 "
    "frames); block streaming serves signal delays of voices only";
typedef std::vector<uint32_t> U;
static bool has_text(const std::string &s, const char *w) { return s.find(w) != std::string::npos; }

// row = In(input) * c
static std::vector<StageInstr> gain(uint32_t input, float c) {
    uint32_t bits;
    std::memcpy(&bits, &c, 4);
    return {ins(S_INPUT, 0, 0, 0, input, 0, 0), ins(S_CONST, 1, 0, 0, bits, 0, 0), ins(S_MUL, 0, 0, 1, 0, 0, 0)};
}
// x = In(input) + g * Delay(x, d), x in `ring` and in the program's row
static std::vector<StageInstr> echo(uint32_t input, uint32_t ring, uint32_t d, float g) {
    uint32_t bits;
    std::memcpy(&bits, &g, 4);
    return {ins(S_INPUT, 0, 0, 0, input, 0, 0), ins(S_READ, 1, 0, 0, 0, ring, d), ins(S_CONST, 2, 0, 0, bits, 0, 0),
            ins(S_MUL, 1, 1, 2, 0, 0, 0),       ins(S_SUM2, 0, 0, 1, 0, 0, 0),    ins(S_STORE, 0, 0, 0, 0, ring, 0)};
}
// row = Delay(ring, d) * In(input)
static std::vector<StageInstr> tap(uint32_t ring, uint32_t d, uint32_t input) {
    return {ins(S_READ, 0, 0, 0, 0, ring, d), ins(S_INPUT, 1, 0, 0, input, 0, 0), ins(S_MUL, 0, 0, 1, 0, 0, 0)};
}
// row = Delay(ring a, da) + Delay(ring b, db)
static std::vector<StageInstr> two_taps(uint32_t a, uint32_t da, uint32_t b, uint32_t db) {
    return {ins(S_READ, 0, 0, 0, 0, a, da), ins(S_READ, 1, 0, 0, 0, b, db), ins(S_SUM2, 0, 0, 1, 0, 0, 0)};
}

// a plan without a bank launch: `rows` output rows, input slots 0 .. n_in - 1, every stream option but FR_STREAM_BUS
static Built voiceless(uint32_t rows, uint32_t n_in, bool feedback) {
    Built b;
    b.env.n_slots = rows;
    b.env.effects = b.env.inputs = b.env.loops = b.env.dyn = b.env.history = true;
    b.sp.feedback = feedback;
    for (uint32_t s = 0; s < n_in; ++s) b.sp.input_slots.push_back(s);
    return b;
}
// tests/stream_fx_cases.py comb_5, and tap_behind with the comb's delay as a parameter
static Built comb_plan(uint32_t d) {
    Built b = voiceless(1, 2, true);
    b.sp.n_rings = 1;
    b.program(echo(1, 0, d, 0.5f), 0, NO_RING, 0);
    return b;
}
static Built tap_behind_plan() {
    Built b = voiceless(2, 3, true);
    b.sp.n_rings = 1;
    b.program(echo(1, 0, 3, 0.6f), 0, NO_RING, 0);
    b.program(tap(0, 2, 2), 0, NO_RING, 1);
    return b;
}
static Built bus_of_combs_plan() {
    Built b = voiceless(3, 3, true);
    b.env.bus = true;
    b.sp.n_rings = 2;
    b.program(echo(1, 0, 3, 0.6f), 0, NO_RING, 0);
    b.program(echo(2, 1, 4, -0.5f), 0, NO_RING, 1);
    b.program(two_taps(0, 1, 1, 2), 0, NO_RING, 2);
    return b;
}

static void test_rule() {
    {   // one level of three programs that read no ring: three groups, three segments, each program in its own
        Built b = voiceless(3, 3, false);
        for (uint32_t r = 0; r < 3; ++r) b.program(gain(r, 0.5f), 0, NO_RING, (int32_t)r);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.reason.empty() && s.voices == 0 && s.segments == 3 && s.banks.empty() && s.chunks == 0 && s.workgroups() == 0);
        CHECK(s.voice_first == (U{0, 1, 2, 3, 3}) && s.progs == (U{0, 1, 2}) && s.programs_per_voice() == (U{1, 1, 1}) && s.bus_programs() == 0);
        CHECK(s.input_slots == (U{0, 1, 2}) && !s.has_loops() && !s.has_hist() && !s.has_dyn());
        b.env.effects = false;                                           // the option off: today's sentence, word for word
        const StreamPlan off = b.plan();
        CHECK(!off.servable && off.reason == OLD && off.segments == 0 && off.voice_first.empty());
        b.env.effects = true;
        b.env.inputs = false;                                            // every other check applies, with its own text
        CHECK(!b.plan().servable && b.plan().reason == "a program reads input slot 1; block streaming feeds slot 0 only");
    }
    {   // slot 0 stays row 0 of every block, whether or not a program reads it
        Built b = voiceless(1, 3, false);
        b.program(gain(2, 0.5f), 0, NO_RING, 0);
        CHECK(b.plan().servable && b.plan().input_slots == (U{0, 2}) && stream_launch(b.sp, b.plan()).n_rows == 2);
    }
    {   // more groups than workgroups: group g runs in segment g % segments, in the order of `run` inside a segment
        Built b = voiceless(10, 1, false);
        for (uint32_t r = 0; r < 10; ++r) b.program(gain(0, 0.5f), 0, NO_RING, (int32_t)r);
        b.env.device_cus = 4;
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.segments == 4 && s.voice_first == (U{0, 3, 6, 8, 10, 10}) && s.progs == (U{0, 4, 8, 1, 5, 9, 2, 6, 3, 7}));
        CHECK(stream_launch(b.sp, s).workgroups == 4);
        b.env.device_cus = 0;                                            // unknown: the kernel's own limit
        CHECK(b.plan().segments == 10);
        b.env.device_cus = 300;
        CHECK(b.plan().segments == 10);
    }
    {   // ... and the kernel's limit itself
        Built b = voiceless(260, 1, false);
        for (uint32_t r = 0; r < 260; ++r) b.program(gain(0, 0.5f), 0, NO_RING, (int32_t)r);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.segments == STREAM_MAX_WGS && s.voice_first.size() == STREAM_MAX_WGS + 2 && s.voice_first[1] == 2 && s.voice_first[4] == 8 &&
              s.voice_first[5] == 9 && s.voice_first[STREAM_MAX_WGS] == 260 && s.progs[0] == 0 && s.progs[1] == 256 && s.progs[2] == 1);
    }
    {   // neither voices nor programs
        Built b = voiceless(1, 1, false);
        CHECK(!b.plan().servable && b.plan().reason == "block streaming of a plan with neither voices nor programs");
    }
    {   // two levels and no fused form: unchanged
        Built b = voiceless(1, 3, false);
        b.sp.n_rings = 1;
        b.program({ins(S_INPUT, 0, 0, 0, 1, 0, 0), ins(S_INPUT, 1, 0, 0, 2, 0, 0), ins(S_MUL, 0, 0, 1, 0, 0, 0)}, 0, 0, -1);
        b.program({ins(S_READ, 0, 0, 0, 0, 0, 10)}, 0, NO_RING, 0);
        b.sp.level_first = {0, 1, 2};
        CHECK(!b.plan().servable && b.plan().reason == NO_FUSED);
    }
    {   // an echo of a block or more is no loop program; a comb is one, of its stride; without FR_STREAM_LOOPS it is refused as ever
        for (uint32_t d : {64u, 100u}) {
            const Built b = comb_plan(d);
            const StreamPlan s = b.plan();
            CHECK(s.servable && s.segments == 1 && s.voice_first == (U{0, 1, 1}) && !s.has_loops() && s.min_ring_delay == d && s.lookback == d);
        }
        for (uint32_t d : {1u, 5u, 63u}) {
            Built b = comb_plan(d);
            const StreamPlan s = b.plan();
            CHECK(s.servable && s.segments == 1 && s.loop_stride == (U{d}) && s.min_ring_delay == d);
            b.env.loops = false;
            CHECK(!b.plan().servable && b.plan().reason == "a program's ring is read " + std::to_string(d) + " frames back; a streamed block needs delays of at least 64 frames");
        }
    }
    {   // the tap behind a loop follows the loop's group: one segment, in the order of `run`; so does a row copy of the loop's ring
        Built b = tap_behind_plan();
        StreamPlan s = b.plan();
        CHECK(s.servable && s.segments == 1 && s.voice_first == (U{0, 2, 2}) && s.progs == (U{0, 1}) && s.loop_stride == (U{3, 0}) && s.min_ring_delay == 2);
        b.env.n_slots = 3;
        b.program(follow(0), 0, NO_RING, 2);                             // a row copy (a feedback plan's post program)
        b.sp.fused_count = 2; b.sp.post_first = 2; b.sp.post_count = 1;
        s = b.plan();
        CHECK(s.servable && s.segments == 1 && s.voice_first == (U{0, 3, 3}) && s.progs == (U{0, 1, 2}));
        // a second comb next to it opens a second group; its own tap follows that one
        b.env.n_slots = 5;
        b.sp.n_rings = 2;
        b.sp.post_count = 0;
        b.program(echo(2, 1, 4, -0.5f), 0, NO_RING, 3);
        b.program(tap(1, 1, 1), 0, NO_RING, 4);
        b.sp.fused_count = 5; b.sp.post_first = 5;
        s = b.plan();                                                    // (the copy is now a fused program that reads ring 0 at the current frame)
        CHECK(s.servable && s.segments == 2 && s.voice_first == (U{0, 3, 5, 5}) && s.progs == (U{0, 1, 2, 3, 4}) && s.loop_stride == (U{3, 0, 0, 4, 0}));
        b.env.device_cus = 1;                                            // one workgroup: both groups in it, still in the order of `run`
        s = b.plan();
        CHECK(s.servable && s.segments == 1 && s.voice_first == (U{0, 5, 5}) && s.progs == (U{0, 1, 2, 3, 4}));
    }
    {   // a program that would follow two groups: a bus program with FR_STREAM_BUS -- no bank ring anywhere --, refused without
        Built b = bus_of_combs_plan();
        StreamPlan s = b.plan();
        CHECK(s.servable && s.segments == 2 && s.voice_first == (U{0, 1, 2, 3}) && s.bus_programs() == 1 && s.progs == (U{0, 1, 2}) && s.loop_stride == (U{3, 4, 0}));
        CHECK(stream_launch(b.sp, s).workgroups == 2);
        b.env.bus = false;
        CHECK(!b.plan().servable &&
              b.plan().reason == "a program reads program groups 0 and 1 in the same block (a mix bus across program groups); each streamed program follows one program group");
        b.env.bus = true;
        // what reads a bus program's ring below a block is a bus program too, and so is the row copy of that ring
        b.env.n_slots = 5;
        b.sp.n_rings = 3;
        b.sp.progs[2].dst_ring = 2;
        b.program(tap(2, 1, 1), 0, NO_RING, 3);
        b.program(follow(2), 0, NO_RING, 4);
        b.sp.fused_count = 4; b.sp.post_first = 4; b.sp.post_count = 1;
        s = b.plan();
        CHECK(s.servable && s.segments == 2 && s.voice_first == (U{0, 1, 2, 5}) && s.bus_programs() == 3 && s.progs == (U{0, 1, 2, 3, 4}));
        b.env.device_cus = 1;                                            // the bus segment stays behind the one segment
        s = b.plan();
        CHECK(s.servable && s.segments == 1 && s.voice_first == (U{0, 2, 5}) && s.bus_programs() == 3);
    }
    {   // reads a block or more back bind nothing: of any ring, and of any slot's history
        Built b = bus_of_combs_plan();
        b.env.bus = false;
        b.sp.instrs[b.sp.progs[2].first_instr] = ins(S_READ, 0, 0, 0, 0, 0, 64);
        b.sp.instrs[b.sp.progs[2].first_instr + 1] = ins(S_READ, 1, 0, 0, 0, 1, 100);
        StreamPlan s = b.plan();
        CHECK(s.servable && s.segments == 3 && s.voice_first == (U{0, 1, 2, 3, 3}) && s.bus_programs() == 0 && s.lookback == 100);
        b.sp.instrs[b.sp.progs[2].first_instr] = ins(S_READ_INPUT, 0, 0, 0, 1, 0, 3);
        b.sp.instrs[b.sp.progs[2].first_instr + 1] = ins(S_READ_INPUT, 1, 0, 0, 2, 0, 0);
        s = b.plan();
        CHECK(s.servable && s.segments == 3 && s.bus_programs() == 0 && s.hist_reads == 2 && s.input_lookback == 3);
        b.env.history = false;
        CHECK(!b.plan().servable && has_text(b.plan().reason, "a program uses S_READ_INPUT (a delayed read of an input row), which block streaming does not serve yet"));
    }
    {   // Delays by a signal amount: of an input row with a proven bound served (FR_STREAM_DYN, FR_STREAM_HISTORY); of a ring that a
        // program stores refused with today's text
        Built b = voiceless(1, 3, false);
        b.program({ins(S_INPUT, 1, 0, 0, 2, 0, 0), ins(S_READ_INPUT_DYN, 0, 1, 0, 1, 48, 0xFFFFFFFFu)}, 0, NO_RING, 0);
        StreamPlan s = b.plan();
        CHECK(s.servable && s.segments == 1 && s.hist_dyn_reads == 1 && s.input_lookback == 48 && stream_launch(b.sp, s).hist_cap == 128);
        b.env.dyn = false;
        CHECK(!b.plan().servable && b.plan().reason == "a program uses S_READ_INPUT_DYN (a Delay by a signal amount), which block streaming does not serve yet");
        b.env.dyn = true;
        b.sp.instrs[1].buf = 0xFFFFFFFFu;
        CHECK(!b.plan().servable && has_text(b.plan().reason, "without a proven bound"));
        Built c = voiceless(2, 4, false);
        c.sp.n_rings = 1;
        c.program({ins(S_INPUT, 0, 0, 0, 1, 0, 0), ins(S_INPUT, 1, 0, 0, 2, 0, 0), ins(S_MUL, 0, 0, 1, 0, 0, 0)}, 0, 0, 0);
        c.program({ins(S_INPUT, 1, 0, 0, 3, 0, 0), ins(S_READ_DYN, 0, 1, 0, 0, 0, 48)}, 0, NO_RING, 1);
        CHECK(!c.plan().servable && c.plan().reason == DYN_OF_A_PROGRAM);
        c.env.bus = true;
        CHECK(!c.plan().servable && c.plan().reason == DYN_OF_A_PROGRAM);
        c.env.dyn = false;
        CHECK(!c.plan().servable && c.plan().reason == "a program uses S_READ_DYN (a Delay by a signal amount), which block streaming does not serve yet");
    }
    {   // nine slots; the register budget; one writer per row; a loop's loads
        Built b = voiceless(1, 9, false);
        std::vector<StageInstr> p;
        for (uint32_t s = 0; s < 9; ++s) p.push_back(ins(S_INPUT, (uint8_t)s, 0, 0, s, 0, 0));
        b.program(p, 0, NO_RING, 0);
        CHECK(!b.plan().servable && b.plan().reason == "the programs read 9 distinct input slots (slot 0 included); block streaming feeds at most 8");
        Built r = voiceless(1, 1, false);
        r.program({ins(S_INPUT, (uint8_t)STAGE_REGS, 0, 0, 0, 0, 0)}, 0, NO_RING, 0);
        CHECK(!r.plan().servable && r.plan().reason == "a program needs more registers than the streamed interpreter has");
        Built w = voiceless(2, 1, false);
        w.program(gain(0, 0.5f), 0, NO_RING, 0);
        w.program(gain(0, 0.25f), 0, NO_RING, 0);
        CHECK(!w.plan().servable && w.plan().reason == "output row 0 is written by 2 streamed programs or voices (exactly one is needed)");
        w.sp.progs[1].out_row = 2;
        CHECK(!w.plan().servable && w.plan().reason == "a program writes output row 2 of 2");
        Built l = comb_plan(5);
        std::vector<StageInstr> many = echo(1, 0, 5, 0.5f);
        for (uint32_t k = 0; k < STREAM_LOOP_LOADS - 1; ++k) many.insert(many.begin(), ins(S_INPUT, 3, 0, 0, 0, 0, 0));
        l.sp.instrs.clear(); l.sp.progs.clear();
        l.program(many, 0, NO_RING, 0);
        CHECK(!l.plan().servable && l.plan().reason == "a loop program has 33 frame-only loads; block streaming serves at most 32");
    }
    {   // the other refusals that come before the banks are unchanged, and a plan WITH voices is untouched by the option
        Built b = voiceless(1, 1, false);
        b.program(gain(0, 0.5f), 0, NO_RING, 0);
        b.env.pull_mode = true;
        CHECK(b.plan().reason == "block streaming of a renderer in FR_MODE_PULL");
        b.env.pull_mode = false;
        b.env.track_history = true;
        CHECK(b.plan().reason == "block streaming with a track history");
        for (StreamKernel k : {StreamKernel::prog, StreamKernel::bus, StreamKernel::in, StreamKernel::banks, StreamKernel::loops, StreamKernel::general, StreamKernel::dyn}) {
            Built v = kernel_plan(k);
            const StreamPlan off = v.plan();
            v.env.effects = true;
            const StreamPlan on = v.plan();
            CHECK(on.servable && off.servable && on.segments == 0 && on.voices == off.voices && on.voice_first == off.voice_first && on.progs == off.progs &&
                  stream_launch(v.sp, on).kernel == k && stream_launch(v.sp, on).workgroups == stream_launch(v.sp, off).workgroups);
        }
    }
}

// ---- the launch rule, the kernels' numbers, names and forms --------------------------------------------------------------------
struct FormBits { bool progs, bus, rows, table, loops, schedule, dyn, hist, voiceless; };
static bool same_form(StreamForm f, FormBits w) {
    return f.progs == w.progs && f.bus == w.bus && f.rows == w.rows && f.table == w.table && f.loops == w.loops && f.schedule == w.schedule && f.dyn == w.dyn &&
           f.hist == w.hist && f.voiceless == w.voiceless;
}

static void test_launch() {
    CHECK((uint32_t)StreamKernel::fx == (uint32_t)StreamKernel::hist + 2 && (uint32_t)StreamKernel::hist == (uint32_t)StreamKernel::dyn + 2);
    CHECK(std::strcmp(stream_kernel_name(StreamKernel::fx), "bank_stream_fx_kernel") == 0 && stream_kernel_by_plan(StreamKernel::fx) && stream_kernel_named(StreamKernel::fx));
    for (StreamKernel gap : {(StreamKernel)((uint32_t)StreamKernel::dyn + 1), (StreamKernel)((uint32_t)StreamKernel::hist + 1), (StreamKernel)((uint32_t)StreamKernel::fx + 1)})
        CHECK(!stream_kernel_named(gap) && std::strcmp(stream_kernel_name(gap), "") == 0);
    CHECK(std::strcmp(stream_kernel_name(StreamKernel::hist), "bank_stream_hist_kernel") == 0 && std::strcmp(stream_kernel_name(StreamKernel::dyn), "bank_stream_dyn_kernel") == 0);
    // the forms of the nine older kernels, written out: exactly what they were
    CHECK(same_form(stream_form(StreamKernel::plain), {false, false, false, false, false, false, false, false, false}));
    CHECK(same_form(stream_form(StreamKernel::prog), {true, false, false, false, false, false, false, false, false}));
    CHECK(same_form(stream_form(StreamKernel::bus), {true, true, false, false, false, false, false, false, false}));
    CHECK(same_form(stream_form(StreamKernel::in), {true, true, true, false, false, false, false, false, false}));
    CHECK(same_form(stream_form(StreamKernel::banks), {true, true, true, true, false, false, false, false, false}));
    CHECK(same_form(stream_form(StreamKernel::loops), {true, true, true, true, true, false, false, false, false}));
    CHECK(same_form(stream_form(StreamKernel::general), {true, true, true, true, true, true, false, false, false}));
    CHECK(same_form(stream_form(StreamKernel::dyn), {true, true, true, true, true, true, true, false, false}));
    CHECK(same_form(stream_form(StreamKernel::hist), {true, true, true, true, true, true, true, true, false}));
    CHECK(same_form(stream_form(StreamKernel::fx), {true, true, true, false, true, false, true, true, true}));
    static_assert(stream_form(StreamKernel::fx).voiceless && !stream_form(StreamKernel::fx).table && !stream_form(StreamKernel::fx).schedule, "fx has no bank");
    {   // fx exactly for a plan without a voice; the workgroups are the segments; the history exists whether or not it is read
        const Built g = [] { Built b = voiceless(1, 1, false); b.program(gain(0, 0.5f), 0, NO_RING, 0); return b; }();
        const StreamLaunch l = stream_launch(g.sp, g.plan());
        CHECK(l.kernel == StreamKernel::fx && l.rows_doorbell && l.own_instrs && l.by_plan && !l.bank_table && !l.schedule_table && l.n_rows == 1 && l.workgroups == 1);
        CHECK(l.hist_cap == 64 && l.max_stride == 0 && l.max_loads == 0 && l.max_stores == 0);
        const Built c = comb_plan(5);
        const StreamLaunch m = stream_launch(c.sp, c.plan());
        CHECK(m.kernel == StreamKernel::fx && m.n_rows == 2 && m.workgroups == 1 && m.hist_cap == 64 && m.max_stride == 5 && m.max_loads == 2 && m.max_stores == 1);
        const Built t = tap_behind_plan();
        const StreamLaunch n = stream_launch(t.sp, t.plan());
        CHECK(n.kernel == StreamKernel::fx && n.n_rows == 3 && n.workgroups == 1 && n.max_stride == 3);
        Built h = voiceless(1, 2, false);
        h.program({ins(S_READ_INPUT, 0, 0, 0, 1, 0, 100)}, 0, NO_RING, 0);
        CHECK(stream_launch(h.sp, h.plan()).kernel == StreamKernel::fx && stream_launch(h.sp, h.plan()).hist_cap == 256);
    }
    for (StreamKernel k : {StreamKernel::prog, StreamKernel::bus, StreamKernel::in, StreamKernel::banks, StreamKernel::loops, StreamKernel::general, StreamKernel::dyn}) {
        Built b = kernel_plan(k);                                        // a plan with voices never gets it
        b.env.effects = true;
        const StreamLaunch l = stream_launch(b.sp, b.plan());
        CHECK(b.plan().voices != 0 && l.kernel == k && l.hist_cap == 0);
    }
}

// ---- stream_launch_check of the fx form -------------------------------------------------------------------------------------------
static float some_floats[1];
static uint32_t some_words[4];
static StageInstr some_instrs[1];
static StageProg some_progs[1];
static BankStreamInCtl some_ctl;
static BankStreamInDev some_dev;

static StreamLaunchArgs minimal() {   // three segments; no parameters, rows, workspace, tickets or tables
    StreamLaunchArgs x{};
    x.a.out = some_floats;
    x.a.n_voices = 3; x.a.leaf_variant = 1;
    x.p.instrs = some_instrs; x.p.progs = some_progs; x.p.voice_first = some_words; x.p.rings = some_floats; x.p.ring_mask = 63; x.p.n_rings = 1;
    x.h.hist = some_floats; x.h.mask = 63;
    x.n_rows = 2; x.max_stride = 5; x.max_loads = 2; x.max_stores = 1;
    x.ctl_dev = &some_ctl; x.dev = &some_dev;
    return x;
}

static void test_check() {
    const StreamKernel X = StreamKernel::fx;
    CHECK(stream_launch_check(X, minimal()) == 3);
    auto broken = [&](auto &&apply) { StreamLaunchArgs x = minimal(); apply(x); return stream_launch_check(X, x); };
    // the segment count
    CHECK(broken([](StreamLaunchArgs &x) { x.a.n_voices = 0; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.a.n_voices = BANK_STREAM_WGS + 1; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.a.n_voices = BANK_STREAM_WGS; }) == BANK_STREAM_WGS);
    CHECK(broken([](StreamLaunchArgs &x) { x.a.n_voices = 1; }) == 1);
    // what it checks as the hist form does
    CHECK(broken([](StreamLaunchArgs &x) { x.a.leaf_variant = 0; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.a.out = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.ctl_dev = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.dev = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.n_rows = 0; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.n_rows = BANK_STREAM_ROWS + 1; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.n_rows = BANK_STREAM_ROWS; }) == 3);
    CHECK(broken([](StreamLaunchArgs &x) { x.h.hist = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.h.mask = 62; }) == 0);                      // not 2^n - 1
    CHECK(broken([](StreamLaunchArgs &x) { x.h.mask = 31; }) == 0);                      // a capacity below a block
    CHECK(broken([](StreamLaunchArgs &x) { x.h.mask = 0; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.h.mask = ~0ull; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.h.mask = 255; }) == 3);
    CHECK(broken([](StreamLaunchArgs &x) { x.max_stride = BANK_STREAM_LOOP_MAX_STRIDE + 1; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.max_loads = BANK_STREAM_LOOP_LOADS + 1; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.max_stores = BANK_STREAM_LOOP_STORES + 1; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.p.n_rings = 0; }) == 0);                    // a loop lives in a ring
    CHECK(broken([](StreamLaunchArgs &x) { x.p.voice_first = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.p.ring_mask = 62; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.p.rings = nullptr; }) == 0);
    CHECK(broken([](StreamLaunchArgs &x) { x.p.ring_mask = 31; }) == 0);
    // a plan without rings or loops (a gain) is taken
    CHECK(broken([](StreamLaunchArgs &x) { x.p.n_rings = 0; x.p.rings = nullptr; x.p.ring_mask = 0; x.max_stride = x.max_loads = x.max_stores = 0; }) == 3);
    // what it does not read: a bank's fields, the tables, bank_to_ring
    CHECK(broken([](StreamLaunchArgs &x) { x.a.log2_p = 3; x.a.chunk_log2 = 9; x.p.bank_to_ring = 1; x.t.n_banks = 77; x.g.mask = 0xFFFFu; }) == 3);
    // the same arguments are no launch of any kernel with voices (no parameters, no rows), and the gaps between the numbers are no kernel
    for (StreamKernel k : {StreamKernel::plain, StreamKernel::prog, StreamKernel::bus, StreamKernel::in, StreamKernel::banks, StreamKernel::loops, StreamKernel::general,
                           StreamKernel::dyn, StreamKernel::hist})
        CHECK(stream_launch_check(k, minimal()) == 0);
    CHECK(stream_launch_check((StreamKernel)((uint32_t)StreamKernel::dyn + 1), minimal()) == 0);
    CHECK(stream_launch_check((StreamKernel)((uint32_t)StreamKernel::hist + 1), minimal()) == 0);
    CHECK(stream_launch_check((StreamKernel)((uint32_t)StreamKernel::fx + 1), minimal()) == 0);
    CHECK(stream_launch_check(StreamKernel::none, minimal()) == 0 && stream_launch_check((StreamKernel)0xFFFFFFFFu, minimal()) == 0);
}

// ---- one segment's block as plain loops ---------------------------------------------------------------------------------------
// kernels.hip stream_run_programs_loops in the voiceless form: the wave of a segment runs its programs in order on the block's n
// frames at `head`; a program of stride 0 lane = frame, all 64 lanes in step (stream_run_programs), a loop program in three
// phases (stream_run_loop_program).  Rings are [ring][mask + 1], the block's rows [row][64] with +0.0 beyond n, out [row][64].
// Loads of lanes beyond the block read whatever the rings hold there, as the kernel's do; only live lanes store.
struct SegmentModel {
    std::vector<float> rings;
    uint64_t mask;
    float regs[STAGE_REGS][64], ldt[STREAM_LOOP_LOADS][64], stt[STREAM_LOOP_STORES][64];
    SegmentModel(uint32_t n_rings, uint64_t cap) : rings((size_t)n_rings * cap, 0.0f), mask(cap - 1) {}
    float &ring(uint32_t r, uint64_t frame) { return rings[(size_t)r * (mask + 1) + (frame & mask)]; }
    float load(const StageInstr &in, uint64_t frame, const float (*rows)[64], uint32_t lane) {   // stream_prog_load, without a history
        switch (in.op) {
        case S_CONST: { float v; std::memcpy(&v, &in.imm, 4); return v; }
        case S_INPUT: return rows[in.imm & 7u][lane];
        case S_READ: return frame >= in.d_lo ? ring(in.buf, frame - in.d_lo) : 0.0f;
        default: { float v; std::memcpy(&v, &in.imm, 4); return frame >= in.d_lo ? v : 0.0f; }
        }
    }
    static float binop(uint8_t op, float a, float b) { return op == S_SUM2 ? a + b : op == S_MUL ? a * b : op == S_DIV ? a / b : std::fmin(a, b); }
    void plain(const StageProg &pg, const StageInstr *ins, uint64_t head, uint32_t n, const float (*rows)[64], float (*out)[64]) {
        for (uint32_t i = 0; i < pg.n_instr; ++i)
            for (uint32_t lane = 0; lane < 64; ++lane) {
                const StageInstr &in = ins[i];
                if (in.op == S_STORE) { if (lane < n) ring(in.buf, head + lane) = regs[in.a][lane]; continue; }
                regs[in.dst][lane] = in.op >= S_SUM2 && in.op <= S_MIN ? binop(in.op, regs[in.a][lane], regs[in.b][lane]) : load(in, head + lane, rows, lane);
            }
        for (uint32_t lane = 0; lane < n; ++lane) {
            if (pg.dst_ring != NO_RING) ring(pg.dst_ring, head + lane) = regs[pg.result_reg][lane];
            if (pg.out_row >= 0) out[pg.out_row][lane] = regs[pg.result_reg][lane];
        }
    }
    void loop(const StageProg &pg, const StageInstr *ins, uint64_t head, uint32_t n, const float (*rows)[64], float (*out)[64]) {
        constexpr uint32_t LM = STREAM_LOOP_LOADS - 1, SM = STREAM_LOOP_STORES - 1;
        const uint32_t stride = pg.pad[0];
        for (uint32_t lane = 0; lane < 64; ++lane) {                     // 1. the frame-only loads, lane = frame, live lanes
            uint32_t k = 0;
            for (uint32_t i = 0; i < pg.n_instr; ++i) {
                const StageInstr &in = ins[i];
                if (in.op != S_INPUT && in.op != S_READ) continue;
                const bool inside = in.op == S_READ && in.imm != 0u && lane >= in.d_lo;
                ldt[k++ & LM][lane] = lane < n && !inside ? load(in, head + lane, rows, lane) : 0.0f;
            }
        }
        for (uint32_t r = 0; r < stride; ++r)                            // 2. a lane per residue
            for (uint32_t f = r; f < n; f += stride) {
                uint32_t k = 0;
                for (uint32_t i = 0; i < pg.n_instr; ++i) {
                    const StageInstr &in = ins[i];
                    float v;
                    switch (in.op) {
                    case S_CONST: std::memcpy(&v, &in.imm, 4); break;
                    case S_INPUT: v = ldt[k++ & LM][f]; break;
                    case S_READ: {
                        const uint32_t slot = k++ & LM;
                        v = in.imm != 0u && f >= in.d_lo ? stt[(in.imm - 1u) & SM][(f - in.d_lo) & 63u] : ldt[slot][f];
                        break;
                    }
                    case S_STORE: stt[(in.imm - 1u) & SM][f] = regs[in.a][f]; continue;
                    default: v = binop(in.op, regs[in.a][f], regs[in.b][f]); break;
                    }
                    regs[in.dst][f] = v;
                }
            }
        for (uint32_t i = 0; i < pg.n_instr; ++i)                        // 3. the block's stores, lane = frame
            if (ins[i].op == S_STORE)
                for (uint32_t lane = 0; lane < n; ++lane) ring(ins[i].buf, head + lane) = stt[(ins[i].imm - 1u) & SM][lane];
        for (uint32_t lane = 0; lane < n; ++lane)
            if (pg.out_row >= 0) out[pg.out_row][lane] = regs[pg.result_reg][lane];
    }
};

static uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

// The plan's one segment through the model, block by block from frame 0, against `dense(frame, rows of all frames so far)`.
template <class Dense>
static void run_segment(const Built &b, uint32_t n_out, Dense &&dense) {
    const StreamPlan s = b.plan();
    CHECK(s.servable && s.segments == 1);
    if (!s.servable) return;
    // the stream's own copy of the programs (engine.cpp begin_program_stream): S_INPUT by streamed row, a loop program prepared
    std::vector<StageProg> progs;
    std::vector<std::vector<StageInstr>> own;
    for (size_t i = 0; i < s.progs.size(); ++i) {
        StageProg pg = b.sp.progs[s.progs[i]];
        std::vector<StageInstr> in(b.sp.instrs.begin() + pg.first_instr, b.sp.instrs.begin() + pg.first_instr + pg.n_instr);
        for (StageInstr &x : in)
            if (x.op == S_INPUT) x.imm = (uint32_t)(std::find(s.input_slots.begin(), s.input_slots.end(), b.sp.input_slots[x.imm]) - s.input_slots.begin());
        if (s.loop_stride[i] != 0) CHECK(stream_loop_prepare(pg, in) && pg.pad[0] == s.loop_stride[i]);
        progs.push_back(pg);
        own.push_back(in);
    }
    const uint32_t n_rows = (uint32_t)s.input_slots.size();
    SegmentModel m(b.sp.n_rings, 128);                                   // the look-back (< 64) and a block, a power of two
    std::mt19937 rng(0xF5);
    std::uniform_real_distribution<float> u(-1.5f, 1.5f);
    std::vector<std::vector<float>> all(n_rows);
    uint64_t head = 0;
    int bad = 0;
    for (int block = 0; block < 24; ++block) {
        const uint32_t n = block < 2 ? 64 : block == 2 ? 1 : 1 + rng() % 64;
        float rows[8][64] = {}, out[4][64];
        for (uint32_t r = 0; r < n_rows; ++r)
            for (uint32_t i = 0; i < n; ++i) all[r].push_back(rows[r][i] = r == 0 ? (float)(head + i) : u(rng));
        for (auto &o : out) for (float &v : o) v = std::nanf("");
        for (uint32_t pi = s.voice_first[0]; pi < s.voice_first[1]; ++pi)
            if (progs[pi].pad[0]) m.loop(progs[pi], own[pi].data(), head, n, rows, out);
            else m.plain(progs[pi], own[pi].data(), head, n, rows, out);
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t r = 0; r < n_out; ++r)
                if (bits(out[r][i]) != bits(dense(r, head + i, all))) ++bad;
        head += n;
    }
    CHECK(bad == 0 && head > 300);
}

static void test_segment_model() {
    {   // comb_5: x[t] = in1[t] + 0.5 * x[t - 5]
        std::vector<float> x;
        run_segment(comb_plan(5), 1, [&](uint32_t, uint64_t t, const std::vector<std::vector<float>> &in) {
            if (x.size() <= t) {
                const float m = (t >= 5 ? x[t - 5] : 0.0f) * 0.5f;
                x.push_back(in[1][t] + m);
            }
            return x[t];
        });
    }
    {   // one_pole, the stride at which one lane walks the whole block
        std::vector<float> x;
        run_segment(comb_plan(1), 1, [&](uint32_t, uint64_t t, const std::vector<std::vector<float>> &in) {
            if (x.size() <= t) {
                const float m = (t >= 1 ? x[t - 1] : 0.0f) * 0.5f;
                x.push_back(in[1][t] + m);
            }
            return x[t];
        });
    }
    {   // tap_behind: row 0 = x[t] = in1[t] + 0.6 * x[t - 3]; row 1 = x[t - 2] * in2[t]: the tap reads what the loop has just stored
        std::vector<float> x;
        run_segment(tap_behind_plan(), 2, [&](uint32_t row, uint64_t t, const std::vector<std::vector<float>> &in) {
            if (x.size() <= t) {
                const float m = (t >= 3 ? x[t - 3] : 0.0f) * 0.6f;
                x.push_back(in[1][t] + m);
            }
            return row == 0 ? x[t] : (t >= 2 ? x[t - 2] : 0.0f) * in[2][t];
        });
    }
}

int main() {
    test_rule();
    test_launch();
    test_check();
    test_segment_model();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
