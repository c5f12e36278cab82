// streamdyn_tests.cpp -- FR_STREAM_DYN on the host (libfriendship_amd/csrc/streamplan.hpp): the serving rule on hand-built plans
// (a signal delay of a voice's ring, of two voices' with and without FR_STREAM_BUS, of a ring a program stores, inside a loop
// program, of an input row, with an observed bound; the look-back), the launch rule (dyn on top of the cascade, the schedule
// table only with schedule banks, unchanged launches for plans without a signal delay), and a plain-loop model of the
// interpreter's two ops (kernels.hip stream_prog_dyn: the reference's cast, the range test, the masked ring index) on a ring at
// capacity against a direct evaluation over the voice's whole history, in both semantics.  Stand-alone: built and run on the
// CPU with -fsanitize=address,undefined by tests/test_stream_dyn_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
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
static bool has(const std::string &s, const char *w) { return s.find(w) != std::string::npos; }

// ---- hand-built plans (as tests/cpp/streamlaunch_tests.cpp) ---------------------------------------------------------------
struct Built {
    StagedPlan sp;
    std::vector<BankLaunch> banks;
    StreamEnv env;
    Built() { env.programs = true; env.dyn = true; }
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

// voice ring + Delay(`ring`, amount): amount = t * 0.001 in r1 (its bound is the planner's business: `bound` goes to d_lo)
static std::vector<StageInstr> chorus(uint32_t voice_ring, uint32_t ring, uint32_t bound) {
    return {ins(S_READ, 0, 0, 0, 0, voice_ring, 0), ins(S_INPUT, 1, 0, 0, 0, 0, 0), ins(S_READ_DYN, 2, 1, 0, 0, ring, bound), ins(S_SUM2, 0, 0, 2, 0, 0, 0)};
}
static std::vector<StageInstr> step(uint32_t voice_ring) {
    return {ins(S_READ, 0, 0, 0, 0, voice_ring, 0), ins(S_INPUT, 1, 0, 0, 0, 0, 0), ins(S_STEP_DYN, 2, 1, 0, 0x3F400000u, 0, 48), ins(S_SUM2, 0, 0, 2, 0, 0, 0)};
}
static std::vector<StageInstr> follow(uint32_t ring) { return {ins(S_READ, 0, 0, 0, 0, ring, 0)}; }

// two voices of 128 partials behind rings 0 and 1; a chorus of `bound` frames on each
static Built two_choruses(uint32_t bound) {
    Built b;
    b.env.n_slots = 2;
    b.bank(7, true, {0, 1});
    b.sp.n_rings = 2;
    b.sp.input_slots = {0};
    b.program(chorus(0, 0, bound), 0, NO_RING, 0);
    b.program(chorus(1, 1, bound), 0, NO_RING, 1);
    return b;
}

static const char *const OLD = "a program uses S_READ_DYN (a Delay by a signal amount), which block streaming does not serve yet";
static const char *const MIX = " in the same block (a mix bus across voices); each streamed program follows one voice";

static void test_rule() {
    for (uint32_t bound : {0u, 5u, 63u, 64u, 700u, 100000u}) {   // whatever the bound: a read below a block, of the program's own voice
        Built b = two_choruses(bound);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.reason.empty() && s.has_dyn() && s.dyn_reads == 2 && s.dyn_steps == 0);
        CHECK(s.programs_per_voice() == (std::vector<uint32_t>{1, 1}) && s.bus_programs() == 0 && s.progs == (std::vector<uint32_t>{0, 1}));
        CHECK(s.lookback == bound && s.min_ring_delay == 0);     // (min_ring_delay concerns rings that programs store)
        b.env.dyn = false;                                       // without the option: today's refusal, word for word
        const StreamPlan off = b.plan();
        CHECK(!off.servable && off.reason == OLD && !off.has_dyn());
        b.env.dyn = true;
        b.env.bus = true;                                        // one voice per program: FR_STREAM_BUS makes no bus program of it
        CHECK(b.plan().servable && b.plan().bus_programs() == 0);
    }
    {   // the program follows the voice of the signal read, not its number
        Built c;
        c.env.n_slots = 2;
        c.bank(7, true, {0, 1});
        c.sp.n_rings = 2;
        c.sp.input_slots = {0};
        c.program({ins(S_INPUT, 1, 0, 0, 0, 0, 0), ins(S_READ_DYN, 0, 1, 0, 0, 1, 20)}, 0, NO_RING, 0);   // reads voice 1 only
        c.program({ins(S_INPUT, 1, 0, 0, 0, 0, 0), ins(S_READ_DYN, 0, 1, 0, 0, 0, 20)}, 0, NO_RING, 1);   // reads voice 0 only
        const StreamPlan s = c.plan();
        CHECK(s.servable && s.progs == (std::vector<uint32_t>{1, 0}) && s.programs_per_voice() == (std::vector<uint32_t>{1, 1}));
    }
    {   // voice 0 at this frame + a signal delay of voice 1: two voices in one program
        Built b = two_choruses(20);
        b.sp.instrs[2].buf = 1;
        const StreamPlan s = b.plan();
        CHECK(!s.servable && s.reason == std::string("a program reads voices 0 and 1") + MIX);
        b.env.bus = true;                                        // FR_STREAM_BUS: a bus program, the other one stays its voice's
        const StreamPlan t = b.plan();
        CHECK(t.servable && t.bus_programs() == 1 && t.programs_per_voice() == (std::vector<uint32_t>{0, 1}) && t.dyn_reads == 2 && t.lookback == 20);
        CHECK(t.progs == (std::vector<uint32_t>{1, 0}));
        b.sp.instrs[0] = ins(S_READ, 0, 0, 0, 0, 0, 100);        // voice 0 a block or more back: an earlier block's frames, no second voice
        b.env.bus = false;
        const StreamPlan u = b.plan();
        CHECK(u.servable && u.bus_programs() == 0 && u.progs == (std::vector<uint32_t>{0, 1}) && u.lookback == 100);
    }
    {   // two signal reads of two voices, nothing else: the same answers
        Built b = two_choruses(20);
        b.sp.instrs[0] = ins(S_READ_DYN, 0, 1, 0, 0, 1, 9);
        std::swap(b.sp.instrs[0], b.sp.instrs[1]);               // (the amount first)
        CHECK(!b.plan().servable && has(b.plan().reason, MIX));
        b.env.bus = true;
        CHECK(b.plan().servable && b.plan().bus_programs() == 1 && b.plan().dyn_reads == 3);
    }
    {   // S_STEP_DYN touches no memory: served, no look-back, any voice
        Built b;
        b.env.n_slots = 2;
        b.bank(7, true, {0, 1});
        b.sp.n_rings = 2;
        b.sp.input_slots = {0};
        b.program(step(0), 0, NO_RING, 0);
        b.program(step(1), 0, NO_RING, 1);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.dyn_steps == 2 && s.dyn_reads == 0 && s.has_dyn() && s.lookback == 0);
        b.env.dyn = false;
        CHECK(b.plan().reason == "a program uses S_STEP_DYN (a Delay by a signal amount), which block streaming does not serve yet");
    }
    {   // a signal delay of a ring that a program stores: its offset may be 0 frames, only voices' rings are complete
        Built b = two_choruses(20);
        b.env.n_slots = 3;
        b.sp.n_rings = 3;
        b.sp.progs[0].dst_ring = 2;
        b.program({ins(S_INPUT, 1, 0, 0, 0, 0, 0), ins(S_READ_DYN, 0, 1, 0, 0, 2, 500)}, 0, NO_RING, 2);
        for (bool bus : {false, true}) {
            b.env.bus = bus;
            const StreamPlan s = b.plan();
            CHECK(!s.servable && has(s.reason, "S_READ_DYN of a ring that a program stores") && has(s.reason, "signal delays of voices only"));
        }
        b.sp.instrs.back().buf = 7;                              // a ring nobody stores: the same answer, never an index
        CHECK(!b.plan().servable && has(b.plan().reason, "S_READ_DYN of a ring that a program stores"));
    }
    {   // inside a loop program (FR_STREAM_LOOPS): refused with its own reason; next to one: served
        Built b;
        b.env.n_slots = 2;
        b.env.loops = true;
        b.bank(7, true, {0, 1});
        b.sp.feedback = true;
        b.sp.n_rings = 3;
        b.sp.input_slots = {0};
        std::vector<StageInstr> loop{ins(S_READ, 0, 0, 0, 0, 0, 0), ins(S_READ, 1, 0, 0, 0, 2, 1),    ins(S_SUM2, 0, 0, 1, 0, 0, 0),
                                     ins(S_INPUT, 1, 0, 0, 0, 0, 0), ins(S_READ_DYN, 2, 1, 0, 0, 0, 31), ins(S_SUM2, 0, 0, 2, 0, 0, 0), ins(S_STORE, 0, 0, 0, 0, 2, 0)};
        b.program(loop, 0, NO_RING, 0);
        b.program(follow(1), 0, NO_RING, 1);
        const StreamPlan s = b.plan();
        CHECK(!s.servable && has(s.reason, "a loop program uses S_READ_DYN") && has(s.reason, "inside a feedback loop shorter than a block"));
        b.env.dyn = false;
        CHECK(b.plan().reason == OLD);
        b.env.dyn = true;
        b.sp.instrs[4] = ins(S_STEP_DYN, 2, 1, 0, 0x3F400000u, 0, 31);
        CHECK(!b.plan().servable && has(b.plan().reason, "a loop program uses S_STEP_DYN"));
        Built c;                                                 // the comb on voice 0, the chorus on voice 1
        c.env = b.env;
        c.bank(7, true, {0, 1});
        c.sp.feedback = true;
        c.sp.n_rings = 3;
        c.sp.input_slots = {0};
        c.program({loop[0], loop[1], loop[2], loop[6]}, 0, NO_RING, 0);
        c.program(chorus(1, 1, 31), 0, NO_RING, 1);
        const StreamPlan t = c.plan();
        CHECK(t.servable && t.has_loops() && t.has_dyn() && t.loop_stride == (std::vector<uint32_t>{1, 0}) && t.dyn_reads == 1 && t.min_ring_delay == 1);
        CHECK(stream_launch(c.sp, t).kernel == StreamKernel::dyn && stream_launch(c.sp, t).max_stride == 1);
    }
    {   // delayed reads of an input row stay refused; with the option on the text names them alone
        for (uint8_t op : {(uint8_t)S_READ_INPUT, (uint8_t)S_READ_INPUT_DYN}) {
            Built b = two_choruses(20);
            b.env.inputs = true;
            b.sp.instrs[2] = ins(op, 2, 1, 0, 0, 0, 20);
            const StreamPlan s = b.plan();
            CHECK(!s.servable && has(s.reason, stage_op_name(op)) && has(s.reason, "(a delayed read of an input row)") && has(s.reason, "a stream keeps no input history"));
            CHECK(!has(s.reason, "a Delay by a signal amount"));
            b.env.dyn = false;
            const StreamPlan off = b.plan();
            CHECK(!off.servable && has(off.reason, op == S_READ_INPUT ? "S_READ_INPUT (a delayed read of the input row), which" : "S_READ_INPUT_DYN (a Delay by a signal amount), which"));
        }
    }
    {   // a bound observed from input rows: a stream stores no rows, the hulls cannot follow
        Built b = two_choruses(400);
        b.sp.observed.push_back({1u, 512u});
        const StreamPlan s = b.plan();
        CHECK(!s.servable && has(s.reason, "a Delay's bound was observed from input rows (FR_DELAY_OBSERVED)"));
        b.env.dyn = false;
        CHECK(b.plan().reason == OLD);
    }
}

// ---- the launch rule ---------------------------------------------------------------------------------------------------
static bool rows_of(const StreamLaunch &l, uint32_t n, bool table, bool schedules) {
    return l.rows_doorbell && l.n_rows == n && l.own_instrs && l.bank_table == table && l.schedule_table == schedules && l.by_plan;
}
static bool same(const StreamLaunch &a, const StreamLaunch &b) {
    return a.kernel == b.kernel && a.rows_doorbell == b.rows_doorbell && a.n_rows == b.n_rows && a.own_instrs == b.own_instrs && a.bank_table == b.bank_table &&
           a.schedule_table == b.schedule_table && a.max_stride == b.max_stride && a.max_loads == b.max_loads && a.max_stores == b.max_stores &&
           a.workgroups == b.workgroups && a.by_plan == b.by_plan;
}

static void test_launch() {
    CHECK(std::strcmp(stream_kernel_name(StreamKernel::dyn), "bank_stream_dyn_kernel") == 0 && stream_kernel_by_plan(StreamKernel::dyn));
    CHECK((uint32_t)StreamKernel::dyn == (uint32_t)StreamKernel::general + 1);
    CHECK(std::strcmp(stream_kernel_name((StreamKernel)((uint32_t)StreamKernel::dyn + 1)), "") == 0);
    {   // one bank, one slot, no schedule bank: rows doorbell, own instructions, bank table, no schedule table
        const Built b = two_choruses(700);
        const StreamLaunch l = stream_launch(b.sp, b.plan());
        CHECK(l.kernel == StreamKernel::dyn && rows_of(l, 1, true, false) && l.max_stride == 0 && l.max_loads == 0 && l.max_stores == 0 && l.workgroups == 2);
    }
    {   // dyn on top of everything: control rows, several banks, a bus segment, a schedule bank
        Built b = two_choruses(20);
        b.env.inputs = b.env.banks = b.env.bus = b.env.general = b.env.loops = true;
        b.env.n_slots = 4;
        b.sp.input_slots = {0, 3};
        b.program({ins(S_INPUT, 0, 0, 0, 1, 0, 0)}, 0, NO_RING, 2);
        b.program({ins(S_READ, 0, 0, 0, 0, 0, 0), ins(S_READ, 1, 0, 0, 0, 1, 0), ins(S_SUM2, 0, 0, 1, 0, 0, 0)}, 0, NO_RING, 3);
        {
            const StreamPlan s = b.plan();
            CHECK(s.servable && s.bus_programs() == 1 && s.input_slots.size() == 2 && !s.has_general());
            CHECK(stream_launch(b.sp, s).kernel == StreamKernel::dyn && rows_of(stream_launch(b.sp, s), 2, true, false));
        }
        b.env.n_slots = 5;
        b.bank(5, false, {4});                                   // 32 partials: a schedule bank (FR_STREAM_GENERAL, FR_STREAM_BANKS)
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.has_general() && s.banks.size() == 2);
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(l.kernel == StreamKernel::dyn && rows_of(l, 2, true, true) && l.workgroups == 3);
        // the same plan without its signal delays: the general kernel, everything else equal
        Built g = b;
        for (StageInstr &i : g.sp.instrs)
            if (i.op == S_READ_DYN) i = ins(S_READ, i.dst, 0, 0, 0, i.buf, 0);
        const StreamPlan t = g.plan();
        CHECK(t.servable && !t.has_dyn());
        StreamLaunch m = stream_launch(g.sp, t);
        CHECK(m.kernel == StreamKernel::general);
        m.kernel = StreamKernel::dyn;
        CHECK(same(l, m));
    }
    {   // plans without a signal delay: the launch does not depend on the option
        for (int kind = 0; kind < 4; ++kind) {
            Built b;
            b.env.n_slots = 2;
            b.env.bus = b.env.inputs = b.env.banks = b.env.loops = b.env.general = true;
            b.bank(kind == 3 ? 5 : 7, true, {0, 1});
            b.sp.n_rings = 3;
            b.sp.input_slots = {0, 2};
            if (kind == 2) b.sp.feedback = true;
            b.program(follow(0), 0, NO_RING, 0);
            if (kind == 0) b.program(follow(1), 0, NO_RING, 1);
            if (kind == 1) b.program({ins(S_READ, 0, 0, 0, 0, 1, 0), ins(S_INPUT, 1, 0, 0, 1, 0, 0), ins(S_MUL, 0, 0, 1, 0, 0, 0)}, 0, NO_RING, 1);
            if (kind == 2) b.program({ins(S_READ, 0, 0, 0, 0, 1, 0), ins(S_READ, 1, 0, 0, 0, 2, 5), ins(S_SUM2, 0, 0, 1, 0, 0, 0), ins(S_STORE, 0, 0, 0, 0, 2, 0)}, 0, NO_RING, 1);
            if (kind == 3) b.program(follow(1), 0, NO_RING, 1);
            const StreamPlan on = b.plan();
            b.env.dyn = false;
            const StreamPlan off = b.plan();
            CHECK(on.servable && off.servable && !on.has_dyn() && on.progs == off.progs && on.voice_first == off.voice_first && on.lookback == off.lookback);
            const StreamLaunch a = stream_launch(b.sp, on), c = stream_launch(b.sp, off);
            CHECK(same(a, c));
            const StreamKernel want[] = {StreamKernel::prog, StreamKernel::in, StreamKernel::loops, StreamKernel::general};
            CHECK(a.kernel == want[kind]);
        }
    }
}

// ---- the two ops: the interpreter's arithmetic as plain loops against the reference's definition --------------------------
// kernels.hip delay_frames: the amount -> frames; false: the output is 0 (the amount is >= 2^64; sparkle: negative or NaN)
static bool delay_frames(float d, uint64_t &frames, bool sparkle) {
    if (d >= 18446744073709551616.0f) return false;
    if (sparkle && !(d >= 0.0f)) return false;
    frames = (d < 0.0f || d != d) ? 0ull : (uint64_t)d;
    return true;
}
// kernels.hip stream_prog_dyn; `ring` has ring_mask + 1 floats (ASan watches both ends)
static float model(const float *ring, uint64_t ring_mask, bool sparkle, uint8_t op, uint32_t imm, float amount, uint64_t frame) {
    uint64_t fr;
    if (!delay_frames(amount, fr, sparkle) || frame < fr) return 0.0f;
    if (op == S_STEP_DYN) { float v; std::memcpy(&v, &imm, 4); return v; }
    return ring[(frame - fr) & ring_mask];
}
// the definition (the reference's Delay, the sparkle renderer's): the source `frames` back in its whole history, 0 before frame 0
static float direct(const std::vector<float> &history, float constant, bool of_constant, bool sparkle, float amount, uint64_t frame) {
    if (amount >= 18446744073709551616.0f) return 0.0f;
    if (sparkle && (amount < 0.0f || std::isnan(amount))) return 0.0f;
    const double whole = (std::isnan(amount) || amount < 0.0f) ? 0.0 : std::floor((double)amount);   // (exact: a float's floor is a double)
    if (whole > (double)frame) return 0.0f;
    return of_constant ? constant : history[frame - (uint64_t)whole];
}
static uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

static void test_ops() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    for (uint32_t bound : {48u, 100u, 700u}) {
        uint64_t cap = 64;                                       // the engine's ring: a power of two that holds the bound and a block
        while (cap < (uint64_t)bound + STREAM_BLOCK) cap <<= 1;
        const float amounts[] = {-1.0f, -0.0f, 0.0f, 0.5f, 1.0f, 63.0f, 64.0f, 65.0f, (float)bound, 2147483648.0f, 9223372036854775808.0f, 18446744073709551616.0f,
                                 inf, -inf, nan};
        for (uint64_t frame : {0ull, 1ull, 63ull, 64ull, 1000ull}) {
            std::vector<float> history(frame + 1);
            for (uint64_t t = 0; t <= frame; ++t) history[t] = 1.0f + (float)t * 0.25f;
            std::vector<float> ring(cap, nan);                   // what the stream has stored by now: the last `cap` frames, each at t & mask
            for (uint64_t t = frame + 1 > cap ? frame + 1 - cap : 0; t <= frame; ++t) ring[t & (cap - 1)] = history[t];
            for (bool sparkle : {false, true})
                for (float amount : amounts) {
                    uint64_t fr = 0;
                    const bool cast = delay_frames(amount, fr, sparkle);
                    const float r = model(ring.data(), cap - 1, sparkle, S_READ_DYN, 0, amount, frame);
                    const float s = model(ring.data(), cap - 1, sparkle, S_STEP_DYN, bits(0.75f), amount, frame);
                    CHECK(bits(s) == bits(direct(history, 0.75f, true, sparkle, amount, frame)));
                    if (!cast || fr > frame || fr <= bound) {    // within the bound (or no read at all): the value is the definition's
                        const float want = direct(history, 0.0f, false, sparkle, amount, frame);
                        if (bits(r) != bits(want)) std::printf("  bound %u frame %llu amount %a sparkle %d: got %a want %a\n", bound, (unsigned long long)frame, amount, (int)sparkle, r, want);
                        CHECK(bits(r) == bits(want));
                    } else {                                     // past the bound: an address inside the ring all the same (the planner's proof is for the value)
                        CHECK(bits(r) == bits(ring[(frame - fr) & (cap - 1)]));
                    }
                }
        }
    }
    uint64_t fr = 7;                                             // the cast itself
    CHECK(delay_frames(-1.0f, fr, false) && fr == 0 && !delay_frames(-1.0f, fr, true));
    CHECK(delay_frames(nan, fr, false) && fr == 0 && !delay_frames(nan, fr, true));
    CHECK(delay_frames(-0.0f, fr, true) && fr == 0 && delay_frames(0.5f, fr, true) && fr == 0 && delay_frames(64.99f, fr, true) && fr == 64);
    CHECK(delay_frames(9223372036854775808.0f, fr, false) && fr == 1ull << 63);
    CHECK(delay_frames(18446742974197923840.0f, fr, false) && fr == 0xFFFFFF0000000000ull);   // the largest float below 2^64
    CHECK(!delay_frames(18446744073709551616.0f, fr, false) && !delay_frames(inf, fr, false) && delay_frames(-inf, fr, false) && fr == 0);
}

int main() {
    test_rule();
    test_launch();
    test_ops();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
