// streamtaps_tests.cpp -- FR_STREAM_TAPS on the host (libfriendship_amd/csrc/streamplan.hpp): the serving rule on hand-built plans
// WITHOUT feedback and without a fused form (the run form in level order, a reader that follows its storer, two storers that make
// a bus program, the mix-bus refusal without FR_STREAM_BUS, a storer that comes later, S_READ_DYN of a ring nobody stores, the
// option off; a plan with a fused form and a feedback plan untouched), the launch rule's choice for each, and a plain-loop model of
// ONE VOICE's chain of programs -- kernels.hip's interpreter, lane = frame: every program's loads of all 64 lanes, then its stores of
// the live lanes, program after program -- over a sequence of blocks against a dense frame-by-frame recurrence: block lengths 64, 1,
// 37, 63, constant delays 1, 63, 64, and a signal amount that hits 0, 63, 64 and the bound on a ring at capacity.
// stream_launch_check is not extended: the tables it receives (StreamProgArgs) are device pointers, which the host cannot read.
// Stand-alone: built and run on the CPU with -fsanitize=address,undefined by tests/test_stream_taps_host.py.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "streamplans.hpp"

static const char *const NO_FUSED = "the plan has no fused form: a program's ring is read less than 64 frames back (or the fused programs exceed the interpreter's budget)";
static const char *const DYN_OF_A_PROGRAM =
    "a program uses S_READ_DYN of a ring that a program stores (a Delay of a computed value by a signal amount, which may be 0 "
    "frames); block streaming serves signal delays of voices only";
static const char *const MIX_BUS = "a program reads voices 0 and 1 in the same block (a mix bus across voices); each streamed program follows one voice";
static const char *const MIX_GROUPS =
    "a program reads program groups 0 and 1 in the same block (a mix bus across program groups); each streamed program follows one program group";
typedef std::vector<uint32_t> U;

// e = In(0) * ring `src` at the current frame (stored to the program's dst_ring)
static std::vector<StageInstr> scaled(uint32_t src) { return {ins(S_INPUT, 1, 0, 0, 0, 0, 0), ins(S_READ, 0, 0, 0, 0, src, 0), ins(S_MUL, 0, 0, 1, 0, 0, 0)}; }
// y = ring at the current frame + ring d frames back
static std::vector<StageInstr> fir(uint32_t ring, uint32_t d) { return {ins(S_READ, 0, 0, 0, 0, ring, 0), ins(S_READ, 1, 0, 0, 0, ring, d), ins(S_SUM2, 0, 0, 1, 0, 0, 0)}; }
// y = Delay(ring a, da) + Delay(ring b, db)
static std::vector<StageInstr> two_taps(uint32_t a, uint32_t da, uint32_t b, uint32_t db) {
    return {ins(S_READ, 0, 0, 0, 0, a, da), ins(S_READ, 1, 0, 0, 0, b, db), ins(S_SUM2, 0, 0, 1, 0, 0, 0)};
}
// y = ring at the current frame + Delay(ring, In(0)) with the bound `bound`
static std::vector<StageInstr> chorus(uint32_t ring, uint32_t bound) {
    return {ins(S_READ, 0, 0, 0, 0, ring, 0), ins(S_INPUT, 1, 0, 0, 0, 0, 0), ins(S_READ_DYN, 2, 1, 0, 0, ring, bound), ins(S_SUM2, 0, 0, 2, 0, 0, 0)};
}

// tests/stream_taps_cases.py env_fir: two voices behind rings 0 and 1; level 1: e_v -> ring 2 + v; level 2: y_v = e_v + Delay(e_v, d) -> row v
static Built env_fir_plan(uint32_t d = 1) {
    Built b;
    b.env.n_slots = 2;
    b.env.taps = true;
    b.bank(7, true, {0, 1});
    b.sp.n_rings = 4;
    b.sp.input_slots = {0};
    b.program(scaled(0), 0, 2, -1);
    b.program(scaled(1), 0, 3, -1);
    b.program(fir(2, d), 0, NO_RING, 0);
    b.program(fir(3, d), 0, NO_RING, 1);
    b.sp.level_first = {0, 0, 2, 4};                                     // (level 0 is the banks': no program)
    return b;
}

static void test_rule() {
    {   // level order; each reader follows its storer: voice 0 runs programs 0 and 2, voice 1 programs 1 and 3
        const Built b = env_fir_plan();
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.reason.empty() && s.voices == 2 && s.levels == 2);
        CHECK(s.progs == (U{0, 2, 1, 3}) && s.voice_first == (U{0, 2, 4, 4}) && s.bus_programs() == 0);
        CHECK(s.short_reads == 4 && s.dyn_ring_reads == 0 && s.min_ring_delay == 0 && s.lookback == 1 && !s.has_dyn() && !s.has_loops());
        CHECK(stream_launch(b.sp, s).kernel == StreamKernel::prog && stream_launch(b.sp, s).workgroups == 2);
        Built off = b;                                                   // the option off: today's sentence, before any instruction is looked at
        off.env.taps = false;
        CHECK(!off.plan().servable && off.plan().reason == NO_FUSED && off.plan().voice_first.empty());
        off.env.bus = off.env.inputs = off.env.banks = off.env.loops = off.env.general = off.env.dyn = off.env.history = off.env.effects = true;
        CHECK(!off.plan().servable && off.plan().reason == NO_FUSED);
    }
    {   // 63 and 64 on either side of the block: only the first is a read below a block
        for (uint32_t d : {63u, 64u}) {
            const Built b = env_fir_plan(d);
            const StreamPlan s = b.plan();
            CHECK(s.servable && s.short_reads == (d < 64 ? 4u : 2u) && s.lookback == d && s.progs == (U{0, 2, 1, 3}));
        }
    }
    {   // a reader of two storers' rings: the mix-bus refusal without FR_STREAM_BUS, a bus program with it -- and so is the reader
        // of the ring that bus program stores
        Built b = env_fir_plan();
        b.env.n_slots = 4;
        b.sp.n_rings = 5;
        b.program(two_taps(2, 1, 3, 2), 0, 4, 2);
        b.program(fir(4, 3), 0, NO_RING, 3);
        b.sp.level_first = {0, 0, 2, 5, 6};
        CHECK(!b.plan().servable && b.plan().reason == MIX_BUS);
        b.env.bus = true;
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.levels == 3 && s.progs == (U{0, 2, 1, 3, 4, 5}) && s.voice_first == (U{0, 2, 4, 6}) && s.bus_programs() == 2);
        CHECK(s.short_reads == 8 && stream_launch(b.sp, s).kernel == StreamKernel::bus);
    }
    {   // a storer that comes later in `run` (no level form of a DAG has one): the "at least 64 frames" sentence
        Built b;
        b.env.n_slots = 1;
        b.env.taps = true;
        b.bank(7, true, {0});
        b.sp.n_rings = 2;
        b.sp.input_slots = {0};
        b.program({ins(S_READ, 0, 0, 0, 0, 1, 5)}, 0, NO_RING, 0);
        b.program(scaled(0), 0, 1, -1);
        b.sp.level_first = {0, 1, 2};
        CHECK(!b.plan().servable && b.plan().reason == "a program's ring is read 5 frames back; a streamed block needs delays of at least 64 frames");
        b.env.bus = true;                                                // (nor does FR_STREAM_BUS serve it: the reader is no bus program)
        CHECK(!b.plan().servable && b.plan().reason == "a program's ring is read 5 frames back; a streamed block needs delays of at least 64 frames");
    }
    {   // S_READ_DYN of a ring an earlier program stores: served with FR_STREAM_DYN, the bound whatever it is a read below a block
        Built b;
        b.env.n_slots = 2;
        b.env.taps = b.env.dyn = true;
        b.bank(7, true, {0, 1});
        b.sp.n_rings = 4;
        b.sp.input_slots = {0};
        b.program(scaled(0), 0, 2, -1);
        b.program(scaled(1), 0, 3, -1);
        b.program(chorus(2, 700), 0, NO_RING, 0);
        b.program(chorus(3, 5), 0, NO_RING, 1);
        b.sp.level_first = {0, 0, 2, 4};
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.progs == (U{0, 2, 1, 3}) && s.dyn_reads == 2 && s.dyn_ring_reads == 2 && s.short_reads == 4 && s.lookback == 700);
        CHECK(stream_launch(b.sp, s).kernel == StreamKernel::dyn && !stream_launch(b.sp, s).schedule_table);
        Built no_dyn = b;
        no_dyn.env.dyn = false;
        CHECK(!no_dyn.plan().servable && no_dyn.plan().reason == "a program uses S_READ_DYN (a Delay by a signal amount), which block streaming does not serve yet");
        Built no_taps = b;
        no_taps.env.taps = false;
        CHECK(!no_taps.plan().servable && no_taps.plan().reason == NO_FUSED);
        Built observed = b;                                              // a bound observed from input rows stays refused
        observed.sp.observed.push_back({0, 700});
        CHECK(!observed.plan().servable && observed.plan().reason.find("a Delay's bound was observed from input rows (FR_DELAY_OBSERVED)") == 0);
        // a signal read of the OTHER voice's program: two voices, the mix-bus refusal; a bus program with FR_STREAM_BUS
        Built cross = b;
        cross.sp.instrs[cross.sp.progs[2].first_instr + 2].buf = 3;
        CHECK(!cross.plan().servable && cross.plan().reason == MIX_BUS);
        cross.env.bus = true;
        CHECK(cross.plan().servable && cross.plan().bus_programs() == 1 && cross.plan().programs_per_voice() == (U{1, 2}) && cross.plan().dyn_ring_reads == 2);
        // of a ring nobody stores, and of one a LATER program stores: the sentence it has always had, never an index
        Built nobody = b;
        nobody.sp.n_rings = 5;
        nobody.sp.instrs[nobody.sp.progs[2].first_instr + 2].buf = 4;
        CHECK(!nobody.plan().servable && nobody.plan().reason == DYN_OF_A_PROGRAM);
        nobody.env.bus = true;
        CHECK(!nobody.plan().servable && nobody.plan().reason == DYN_OF_A_PROGRAM);
        Built later = b;
        later.sp.instrs[later.sp.progs[0].first_instr + 1] = ins(S_READ_DYN, 0, 1, 0, 0, 3, 9);   // program 0 reads ring 3, which program 1 stores
        CHECK(!later.plan().servable && later.plan().reason == DYN_OF_A_PROGRAM);
    }
    {   // a one-level plan: S_READ_DYN of a ring a program of the SAME level stores is not an earlier one's unless it comes first in `run`
        Built b;
        b.env.n_slots = 1;
        b.env.taps = b.env.dyn = true;
        b.bank(7, true, {0});
        b.sp.n_rings = 2;
        b.sp.input_slots = {0};
        b.program({ins(S_INPUT, 1, 0, 0, 0, 0, 0), ins(S_READ_DYN, 0, 1, 0, 0, 1, 9)}, 0, 1, 0);   // reads the ring it stores itself
        CHECK(!b.plan().servable && b.plan().reason == DYN_OF_A_PROGRAM);
    }
    {   // a plan WITH a fused form keeps it; one level is one level
        Built b = two_voices();
        b.env.taps = true;
        const StreamPlan one = b.plan();
        CHECK(one.servable && one.levels == 1 && one.short_reads == 0 && one.progs == (U{0, 1}));
        Built f = two_voices();
        f.env.taps = true;
        f.sp.level_first = {0, 1, 2};                                    // two levels, and a fused form: the fused programs are the run form
        f.sp.fused_first = 1;
        f.sp.fused_count = 1;
        f.env.n_slots = 1;
        f.sp.progs[1].out_row = 0;
        const StreamPlan s = f.plan();
        CHECK(s.servable && s.levels == 1 && s.progs == (U{1}));
    }
    {   // a feedback plan is untouched: the comb of 5 frames with FR_STREAM_LOOPS as ever, without it refused as ever
        Built b = kernel_plan(StreamKernel::loops);
        const StreamPlan before = b.plan();
        b.env.taps = true;
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.progs == before.progs && s.voice_first == before.voice_first && s.loop_stride == before.loop_stride && s.levels == 1 &&
              s.min_ring_delay == before.min_ring_delay && stream_launch(b.sp, s).kernel == StreamKernel::loops);
        b.env.loops = false;
        CHECK(!b.plan().servable && b.plan().reason == "a program's ring is read 5 frames back; a streamed block needs delays of at least 64 frames");
    }
    {   // a plan without a voice (FR_STREAM_EFFECTS): the reader follows its storer's GROUP; two groups make a bus program
        Built b;
        b.env.n_slots = 1;
        b.env.taps = b.env.effects = b.env.inputs = true;
        b.sp.n_rings = 1;
        b.sp.input_slots = {0, 1, 2};
        b.program({ins(S_INPUT, 0, 0, 0, 1, 0, 0), ins(S_INPUT, 1, 0, 0, 2, 0, 0), ins(S_MUL, 0, 0, 1, 0, 0, 0)}, 0, 0, -1);
        b.program({ins(S_READ, 0, 0, 0, 0, 0, 10)}, 0, NO_RING, 0);
        b.sp.level_first = {0, 0, 1, 2};
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.voices == 0 && s.segments == 1 && s.progs == (U{0, 1}) && s.voice_first == (U{0, 2, 2}) && s.levels == 2 && s.short_reads == 1 &&
              s.min_ring_delay == 10);
        CHECK(stream_launch(b.sp, s).kernel == StreamKernel::fx && stream_launch(b.sp, s).workgroups == 1);
        b.env.n_slots = 2;
        b.sp.n_rings = 2;
        b.sp.progs[1].out_row = -1;
        b.sp.progs[1].dst_ring = 1;
        b.sp.instrs[b.sp.progs[1].first_instr] = ins(S_INPUT, 0, 0, 0, 1, 0, 0);   // program 1 now opens a group of its own
        b.program(two_taps(0, 1, 1, 2), 0, NO_RING, 0);
        b.program({ins(S_READ, 0, 0, 0, 0, 1, 0)}, 0, NO_RING, 1);                 // a row copy of ring 1: it follows group 1
        b.sp.level_first = {0, 0, 2, 4};
        CHECK(!b.plan().servable && b.plan().reason == MIX_GROUPS);
        b.env.bus = true;
        const StreamPlan t = b.plan();
        CHECK(t.servable && t.segments == 2 && t.progs == (U{0, 1, 3, 2}) && t.voice_first == (U{0, 1, 3, 4}) && t.bus_programs() == 1);
        b.env.taps = false;
        CHECK(!b.plan().servable && b.plan().reason == NO_FUSED);
    }
}

// ---- a plain-loop model of one voice's chain of programs ------------------------------------------------------------------------
// The wave that finishes the voice: lane = frame head + lane, lanes < n live.  It stores the voice's frames to the voice's ring,
// then runs its programs in order; a program's loads of ALL lanes happen before its stores (one instruction at a time over the
// wave), and every store of a program has landed before the next program's loads (s_waitcnt vmcnt(0)).
struct Model {
    uint64_t cap;
    uint32_t n_rings;
    std::vector<float> rings;
    float regs[STAGE_REGS][64];
    Model(uint32_t n, uint64_t c) : cap(c), n_rings(n), rings((size_t)n * c, 0.0f) {}
    float &at(uint32_t ring, uint64_t frame) { return rings[(size_t)ring * cap + (frame & (cap - 1))]; }
    // (kernels.hip delay_frames, reference semantics: negatives and NaN are 0 frames, floor)
    static uint64_t frames_of(float d) { return (d < 0.0f || d != d) ? 0ull : (uint64_t)d; }
    void run(const StagedPlan &sp, const U &progs, uint64_t head, uint32_t n, const float *input, std::vector<float> &row_out) {
        for (uint32_t pi : progs) {
            const StageProg &pg = sp.progs[pi];
            for (uint32_t i = 0; i < pg.n_instr; ++i) {
                const StageInstr &in = sp.instrs[pg.first_instr + i];
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint64_t frame = head + lane;
                    float v = 0.0f;
                    switch (in.op) {
                    case S_INPUT: v = lane < n ? input[lane] : 0.0f; break;
                    case S_CONST: std::memcpy(&v, &in.imm, 4); break;
                    case S_READ: v = frame >= in.d_lo ? at(in.buf, frame - in.d_lo) : 0.0f; break;
                    case S_READ_DYN: {
                        const uint64_t fr = frames_of(regs[in.a][lane]);
                        v = frame >= fr ? at(in.buf, frame - fr) : 0.0f;
                        break;
                    }
                    case S_SUM2: v = regs[in.a][lane] + regs[in.b][lane]; break;
                    case S_MUL: v = regs[in.a][lane] * regs[in.b][lane]; break;
                    default: CHECK(false); break;
                    }
                    regs[in.dst][lane] = v;
                }
            }
            for (uint32_t lane = 0; lane < n; ++lane) {
                if (pg.dst_ring != NO_RING) at(pg.dst_ring, head + lane) = regs[pg.result_reg][lane];
                if (pg.out_row >= 0) row_out[lane] = regs[pg.result_reg][lane];
            }
        }
    }
};

static float voice_at(uint64_t t) { return std::sin(0.37f * (float)t) + 0.25f * std::sin(1.9f * (float)t); }

static void test_model() {
    // one voice behind ring 0; e = g(t) * voice -> ring 1; y = e + Delay(e, d1) -> ring 2; z = Delay(y, d2) + Delay(y, amount(t)) -> row 0.
    // In(0) is the amount row here AND e's gain (the model's one streamed row), amounts cycling through 0, 63, 64, the bound and
    // values in between; the ring is at capacity: cap == bound + 64
    const uint32_t BOUND = 192;
    const uint64_t CAP = 256;
    const uint32_t lengths[] = {64, 1, 37, 63, 64, 64, 2, 63, 64, 37, 1, 64, 64, 64, 63, 64};
    for (uint32_t d1 : {1u, 63u, 64u})
        for (uint32_t d2 : {1u, 63u, 64u}) {
            Built b;
            b.env.n_slots = 1;
            b.env.taps = b.env.dyn = true;
            b.bank(7, true, {0});
            b.sp.n_rings = 3;
            b.sp.input_slots = {0};
            b.program(scaled(0), 0, 1, -1);
            b.program(fir(1, d1), 0, 2, -1);
            b.program({ins(S_READ, 0, 0, 0, 0, 2, d2), ins(S_INPUT, 1, 0, 0, 0, 0, 0), ins(S_READ_DYN, 2, 1, 0, 0, 2, BOUND), ins(S_SUM2, 0, 0, 2, 0, 0, 0)}, 0, NO_RING, 0);
            b.sp.level_first = {0, 0, 1, 2, 3};
            const StreamPlan s = b.plan();
            CHECK(s.servable && s.levels == 3 && s.progs == (U{0, 1, 2}) && s.lookback == BOUND && stream_hist_cap(s.lookback) == CAP);
            CHECK(stream_launch(b.sp, s).kernel == StreamKernel::dyn);
            if (!s.servable) continue;
            const float amounts[] = {0.0f, 63.0f, 64.0f, (float)BOUND, 1.0f, 17.5f, 100.0f, 191.0f, -3.0f};
            uint64_t total = 0;
            for (uint32_t n : lengths) total += n;
            std::vector<float> in(total), e(total), y(total), z(total);
            for (uint64_t t = 0; t < total; ++t) {                      // the dense recurrence, frame by frame
                in[t] = amounts[(t * 4 + t / 9) % 9];                   // (every nine frames a permutation of the nine amounts)
                e[t] = in[t] * voice_at(t);
                y[t] = e[t] + (t >= d1 ? e[t - d1] : 0.0f);
                const uint64_t fr = Model::frames_of(in[t]);
                z[t] = (t >= d2 ? y[t - d2] : 0.0f) + (t >= fr ? y[t - fr] : 0.0f);
            }
            Model m(3, CAP);
            uint64_t head = 0;
            bool equal = true;
            bool hit[4] = {false, false, false, false};
            for (uint32_t n : lengths) {
                for (uint32_t lane = 0; lane < n; ++lane) m.at(0, head + lane) = voice_at(head + lane);   // the voice's own store
                std::vector<float> out(64, 0.0f);
                m.run(b.sp, U(s.progs.begin() + s.voice_first[0], s.progs.begin() + s.voice_first[1]), head, n, in.data() + head, out);
                for (uint32_t lane = 0; lane < n; ++lane) {
                    equal = equal && std::memcmp(&out[lane], &z[head + lane], 4) == 0;
                    const float a = in[head + lane];
                    if (head + lane >= BOUND) { hit[0] |= a == 0.0f; hit[1] |= a == 63.0f; hit[2] |= a == 64.0f; hit[3] |= a == (float)BOUND; }
                }
                head += n;
            }
            CHECK(equal);
            CHECK(hit[0] && hit[1] && hit[2] && hit[3]);                     // every amount was hit with a full past ...
            CHECK(head > 2 * CAP);                                           // ... and the ring has wrapped twice
        }
}

int main() {
    test_rule();
    test_model();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
