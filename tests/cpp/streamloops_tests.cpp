// streamloops_tests.cpp -- FR_STREAM_LOOPS on the host (libfriendship_amd/csrc/streamplan.hpp): the stride and store-slot helper
// on hand-derived programs, the serving rule on hand-built plans (the one refusal no graph reaches among them), and a
// plain-loop model of the kernel's three phases (kernels.hip stream_run_loop_program), run on the helper's output and compared
// bit for bit with a frame-by-frame evaluation of the plan's own instructions over a ring array -- the sequential loop that the
// reference's recursion defines.  Stand-alone: built and run on the CPU with -fsanitize=address,undefined by
// tests/test_stream_loops_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
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

// x = ring0 + g * Delay(x, d): x in `ring`; the carry annotations are whatever the plan left there
static std::vector<StageInstr> comb(uint32_t voice_ring, uint32_t ring, const std::vector<uint32_t> &delays, bool store) {
    std::vector<StageInstr> p{ins(S_READ, 0, 0, 0, 0, voice_ring, 0)};
    for (uint32_t d : delays) {
        p.push_back(ins(S_READ, 1, 0, 0, 0xFFu, ring, d));
        p.push_back(ins(S_CONST, 2, 0, 0, f32(0.5f), 0, 0));
        p.push_back(ins(S_MUL, 1, 1, 2, 0, 0, 0));
        p.push_back(ins(S_SUM2, 0, 0, 1, 0, 0, 0));
    }
    if (store) p.push_back(ins(S_STORE, 0, 0, 0, 7u, ring, 0));
    return p;
}

static void test_helper() {
    {   // comb(5), the result an explicit store (a feedback plan's form)
        std::vector<StageInstr> p = comb(0, 1, {5}, true);
        StageProg pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_loop_stride(pg, p.data()) == 5 && stream_loop_loads(pg, p.data()) == 2);
        CHECK(stream_loop_prepare(pg, p));
        CHECK(pg.pad[0] == 5 && pg.n_instr == p.size() && p.size() == 6 && pg.dst_ring == NO_RING);
        CHECK(p[0].imm == 0 && p[1].imm == 1 && p[5].op == S_STORE && p[5].imm == 1);
    }
    {   // the same through dst_ring: the helper appends the store
        std::vector<StageInstr> p = comb(0, 1, {5}, false);
        StageProg pg = prog(p, 0, 1, 3);
        CHECK(stream_loop_stride(pg, p.data()) == 5);
        CHECK(stream_loop_prepare(pg, p));
        CHECK(pg.pad[0] == 5 && pg.n_instr == 6 && p.size() == 6 && pg.dst_ring == NO_RING && pg.out_row == 3);
        CHECK(p[5].op == S_STORE && p[5].buf == 1 && p[5].a == 0 && p[5].imm == 1 && p[1].imm == 1);
    }
    const struct { std::vector<uint32_t> d; uint32_t stride; } taps[] = {{{1}, 1}, {{63}, 63}, {{2, 3}, 1}, {{6, 9}, 3}, {{3, 441}, 3}, {{12, 64, 18}, 6}, {{64}, 0},
                                                                         {{441, 128}, 0}};
    for (const auto &t : taps) {
        std::vector<StageInstr> p = comb(0, 1, t.d, true);
        StageProg pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_loop_stride(pg, p.data()) == t.stride);
        CHECK(stream_loop_prepare(pg, p) == (t.stride != 0));
        CHECK(pg.pad[0] == t.stride);
        if (t.stride)
            for (const StageInstr &i : p)
                if (i.op == S_READ) CHECK(i.imm == (i.buf == 1 ? 1u : 0u));   // every own read is marked, the taps of 64 and more too
    }
    {   // a merged component: rings 1 and 2, each read by the other half; slots in store order
        std::vector<StageInstr> p{ins(S_READ, 0, 0, 0, 0, 0, 0), ins(S_READ, 1, 0, 0, 1, 2, 4), ins(S_SUM2, 0, 0, 1, 0, 0, 0), ins(S_STORE, 0, 0, 0, 0, 1, 0),
                                  ins(S_READ, 2, 0, 0, 2, 1, 6), ins(S_READ, 3, 0, 0, 0, 5, 1), ins(S_SUM2, 2, 2, 3, 0, 0, 0), ins(S_STORE, 0, 2, 0, 0, 2, 0)};
        StageProg pg = prog(p, 2, NO_RING, 1);
        CHECK(stream_loop_stride(pg, p.data()) == 2 && stream_stored_rings(pg, p.data()) == (std::vector<uint32_t>{1, 2}));
        CHECK(stream_loop_prepare(pg, p) && pg.pad[0] == 2);
        CHECK(p[1].imm == 2 && p[3].imm == 1 && p[4].imm == 1 && p[5].imm == 0 && p[7].imm == 2);   // ring 5 is somebody else's
    }
    {   // the tiles' limits
        std::vector<StageInstr> p;
        for (uint32_t r = 0; r < STREAM_LOOP_STORES + 1; ++r) {
            p.push_back(ins(S_READ, 0, 0, 0, 0, 1 + r, 1));
            p.push_back(ins(S_STORE, 0, 0, 0, 0, 1 + (r + 1) % (STREAM_LOOP_STORES + 1), 0));
        }
        StageProg pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_loop_stride(pg, p.data()) == 1 && !stream_loop_prepare(pg, p));
        p.resize(2 * STREAM_LOOP_STORES);
        p[2 * STREAM_LOOP_STORES - 1].buf = 1;
        pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_loop_prepare(pg, p) && p.back().imm == STREAM_LOOP_STORES && p[p.size() - 3].imm == STREAM_LOOP_STORES - 1);   // slots in store order
        std::vector<uint32_t> many;
        for (uint32_t k = 0; k < STREAM_LOOP_LOADS; ++k) many.push_back(k + 1);
        p = comb(0, 1, many, true);                                 // LOADS own reads and the voice's ring
        pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_loop_loads(pg, p.data()) == STREAM_LOOP_LOADS + 1 && !stream_loop_prepare(pg, p));
        many.pop_back();
        p = comb(0, 1, many, true);
        pg = prog(p, 0, NO_RING, 0);
        CHECK(stream_loop_prepare(pg, p) && pg.pad[0] == 1);
    }
}

// ---- the rule on hand-built plans -------------------------------------------------------------------------------------------
struct Built {
    StagedPlan sp;
    BankLaunch bank;
    StreamPlan plan(bool loops, bool bus) const {
        StreamEnv env;
        env.n_slots = 2;
        env.loops = loops;
        env.bus = bus;
        return plan_stream(sp, {&bank}, env);
    }
};

// two voices (rings 0, 1); program A = comb(3) of voice 0 in ring 2 that ALSO reads ring 3 `d` frames back; program B = comb(7)
// of voice `b_voice` in ring 3.  `a_first`: A comes before B in the plan.
static Built two_programs(bool a_first, uint32_t d, uint32_t b_voice) {
    Built b;
    b.bank.log2_p = 7;
    b.bank.to_ring = true;
    b.bank.rows = {0, 1};
    b.sp.feedback = true;
    b.sp.n_rings = 4;
    std::vector<StageInstr> A = comb(0, 2, {3}, false);
    A.push_back(ins(S_READ, 1, 0, 0, 0, 3, d));
    A.push_back(ins(S_SUM2, 0, 0, 1, 0, 0, 0));
    A.push_back(ins(S_STORE, 0, 0, 0, 0, 2, 0));
    std::vector<StageInstr> B = comb(b_voice, 3, {7}, true);
    for (int k = 0; k < 2; ++k) {
        const bool is_a = (k == 0) == a_first;
        const std::vector<StageInstr> &p = is_a ? A : B;
        StageProg pg = prog(p, 0, NO_RING, is_a ? 0 : 1);
        pg.first_instr = (uint32_t)b.sp.instrs.size();
        b.sp.instrs.insert(b.sp.instrs.end(), p.begin(), p.end());
        b.sp.progs.push_back(pg);
    }
    b.sp.fused_first = 0;
    b.sp.fused_count = 2;
    b.sp.post_first = 2;
    return b;
}

static void test_rule() {
    {   // B first, on the same voice: A's read of B's ring 2 frames back is a tap behind a loop
        const StreamPlan s = two_programs(false, 2, 0).plan(true, false);
        CHECK(s.servable && s.reason.empty());
        CHECK(s.voice_first == (std::vector<uint32_t>{0, 2, 2, 2}) && s.progs == (std::vector<uint32_t>{0, 1}) && s.loop_stride == (std::vector<uint32_t>{7, 3}));
        CHECK(s.has_loops() && s.min_ring_delay == 2);
    }
    {   // B on the other voice: two voices in one program
        const Built b = two_programs(false, 2, 1);
        const StreamPlan s = b.plan(true, false);
        CHECK(!s.servable && s.reason.find("a program reads voices 0 and 1 in the same block (a mix bus across voices)") == 0);
        const StreamPlan t = b.plan(true, true);                    // with the bus: A is a bus program, and still a loop
        CHECK(t.servable && t.bus_programs() == 1 && t.voice_first == (std::vector<uint32_t>{0, 0, 1, 2}) && t.loop_stride == (std::vector<uint32_t>{7, 3}));
    }
    {   // A first: the ring it reads 2 frames back is stored by a LATER program
        const StreamPlan s = two_programs(true, 2, 0).plan(true, false);
        CHECK(!s.servable && s.reason == "a program's ring is read 2 frames back; a streamed block needs delays of at least 64 frames");
        const StreamPlan t = two_programs(true, 2, 0).plan(true, true);
        CHECK(!t.servable && t.reason == s.reason);
        const StreamPlan u = two_programs(true, 100, 0).plan(true, false);   // a block or more back: an earlier block stored it
        CHECK(u.servable && u.loop_stride == (std::vector<uint32_t>{3, 7}) && u.min_ring_delay == 3);
    }
    {   // the option off: the first short read of a program's ring, as ever
        const StreamPlan s = two_programs(false, 2, 0).plan(false, false);
        CHECK(!s.servable && s.reason == "a program's ring is read 7 frames back; a streamed block needs delays of at least 64 frames" && !s.has_loops());
    }
}

// ---- the three phases against the sequential loop -------------------------------------------------------------------------
constexpr uint32_t CAP = 256, MASK = CAP - 1, N_RINGS = 6, N_ROWS = 3;

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
            switch (in.op) {
            case S_CONST: reg[in.dst] = bitsf(in.imm); break;
            case S_INPUT: reg[in.dst] = rows[in.imm][f]; break;
            case S_READ: reg[in.dst] = t >= in.d_lo ? rings[in.buf * CAP + ((t - in.d_lo) & MASK)] : 0.0f; break;
            case S_STEP: reg[in.dst] = t >= in.d_lo ? bitsf(in.imm) : 0.0f; break;
            case S_STORE: rings[in.buf * CAP + (t & MASK)] = reg[in.a]; break;
            default: reg[in.dst] = binop(in.op, reg[in.a], reg[in.b]); break;
            }
        }
        if (pg.dst_ring != NO_RING) rings[pg.dst_ring * CAP + (t & MASK)] = reg[pg.result_reg];
        out[f] = reg[pg.result_reg];
    }
}

// the kernel's phases as plain loops over the 64 lanes, on the helper's output
static void model(const StageProg &pg, const std::vector<StageInstr> &p, std::vector<float> &rings, const float (*rows)[64], uint64_t head, uint32_t n, float *out) {
    constexpr uint32_t LM = STREAM_LOOP_LOADS - 1, SM = STREAM_LOOP_STORES - 1;
    static float regs[STAGE_REGS][64], ldt[STREAM_LOOP_LOADS][64], stt[STREAM_LOOP_STORES][64];
    const uint32_t stride = pg.pad[0];
    for (uint32_t lane = 0; lane < 64; ++lane) {                    // 1. lane = frame
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
    for (uint32_t lane = 0; lane < stride; ++lane)                  // 2. a lane per residue
        for (uint32_t f = lane; f < n; f += stride) {
            uint32_t k = 0;
            for (const StageInstr &in : p) {
                float v;
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

// A random loop program over: ring 0 (the voice's), rings 1..own (its own), ring 5 (another program's, filled by the test).
static std::vector<StageInstr> random_program(std::mt19937 &rng, uint32_t own, uint32_t stride, bool far_taps, StageProg &pg) {
    auto pick = [&](uint32_t n) { return (uint32_t)(rng() % n); };
    std::vector<StageInstr> p;
    const float gains[] = {0.25f, -0.25f, 0.3f, -0.125f, 0.125f};   // (three reads at the most: the loop decays)
    uint32_t last = 0;
    for (uint32_t part = 0; part < own; ++part) {                   // one merged sub-program per own ring
        uint8_t acc = 0, tmp = 1, c = 2;
        switch (pick(3)) {
        case 0: p.push_back(ins(S_READ, acc, 0, 0, pick(200), 0, 0)); break;
        case 1: p.push_back(ins(S_INPUT, acc, 0, 0, pick(N_ROWS), 0, 0)); break;
        default: p.push_back(ins(S_READ, acc, 0, 0, 0, 5, pick(3) * 37)); break;
        }
        const uint32_t reads = 1 + pick(3);
        for (uint32_t r = 0; r < reads; ++r) {
            uint32_t d = stride * (1 + pick(63 / stride));          // 1..63, a multiple of the stride
            if (r == 0) d = stride;                                 // (so that the gcd is the stride)
            if (far_taps && r == 1) d = 64 + pick(120);
            p.push_back(ins(S_READ, tmp, 0, 0, pick(256), 1 + pick(own), d));
            p.push_back(ins(S_CONST, c, 0, 0, f32(gains[pick(5)]), 0, 0));
            p.push_back(ins(S_MUL, tmp, tmp, c, 0, 0, 0));
            p.push_back(ins(pick(8) ? S_SUM2 : S_MIN, acc, acc, tmp, 0, 0, 0));
        }
        if (pick(4) == 0) {
            p.push_back(ins(S_STEP, tmp, 0, 0, f32(0.0625f), 0, 30 + pick(300)));
            p.push_back(ins(S_SUM2, acc, acc, tmp, 0, 0, 0));
        }
        last = 1 + part;
        if (part + 1 < own || pick(2)) { p.push_back(ins(S_STORE, 0, acc, 0, pick(9), last, 0)); last = 0; }
    }
    pg = prog(p, 0, last ? last : NO_RING, 0);
    return p;
}

static void test_phases() {
    std::mt19937 rng(20260117);
    for (int trial = 0; trial < 60; ++trial) {
        const uint32_t strides[] = {1, 1, 2, 3, 5, 7, 16, 21, 31, 32, 63};
        const uint32_t stride = strides[trial % 11], own = 1 + trial % 2;
        StageProg pg;
        const std::vector<StageInstr> p = random_program(rng, own, stride, trial % 3 == 0, pg);
        StageProg spg = pg;
        std::vector<StageInstr> sp = p;
        CHECK(stream_loop_prepare(spg, sp));
        CHECK(spg.pad[0] == stream_loop_stride(pg, p.data()) && spg.pad[0] >= stride && spg.pad[0] % stride == 0 && spg.pad[0] < 64);
        std::vector<float> ra(N_RINGS * CAP, 0.0f), rb(N_RINGS * CAP, 0.0f);
        uint64_t head = trial % 4 == 0 ? 0 : rng() % 1000;
        bool same = true;
        for (int block = 0; block < 300 && same; ++block) {
            const uint32_t n = 1 + rng() % 64;
            float rows[N_ROWS][64];
            for (auto &row : rows)
                for (float &v : row) v = (float)((int)(rng() % 2001) - 1000) / 512.0f;
            for (uint32_t f = 0; f < n; ++f)                        // the voice's frames and the other program's, stored before this one runs
                for (uint32_t ring : {0u, 5u}) ra[ring * CAP + ((head + f) & MASK)] = rb[ring * CAP + ((head + f) & MASK)] = (float)((int)(rng() % 4001) - 2000) / 1024.0f;
            float oa[64] = {}, ob[64] = {};
            evaluate(pg, p, ra, rows, head, n, oa);
            model(spg, sp, rb, rows, head, n, ob);
            same = std::memcmp(oa, ob, n * sizeof(float)) == 0 && std::memcmp(ra.data(), rb.data(), ra.size() * sizeof(float)) == 0;
            head += n;
        }
        CHECK(same);
        CHECK(head > CAP);                                          // the rings wrapped
    }
}

int main() {
    test_helper();
    test_rule();
    test_phases();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
