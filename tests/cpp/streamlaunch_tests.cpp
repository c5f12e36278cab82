// streamlaunch_tests.cpp -- the launch rule of block streaming on the host (libfriendship_amd/csrc/streamplan.hpp stream_path,
// stream_launch, plain_stream_launch): each of the resident kernels on a hand-built plan (streamplans.hpp) that calls for it, with its
// doorbell form, rows, tables, limits and workgroups; the precedence general > loops > banks > in > bus > prog; the loop limits
// against a direct count over the instructions; the plain path exactly where fr_stream_begin has always taken it; and the
// one-bank chunk dealing against the loop fr_stream_begin used to have.  Stand-alone: built and run on the CPU with
// -fsanitize=address,undefined by tests/test_stream_launch_host.py.
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "streamplans.hpp"

static bool no_limits(const StreamLaunch &l) { return l.max_stride == 0 && l.max_loads == 0 && l.max_stores == 0; }
static bool one_row(const StreamLaunch &l) { return !l.rows_doorbell && l.n_rows == 1 && !l.own_instrs && !l.bank_table && !l.schedule_table && !l.by_plan; }
static bool rows_of(const StreamLaunch &l, uint32_t n, bool table, bool schedules) {
    return l.rows_doorbell && l.n_rows == n && l.own_instrs && l.bank_table == table && l.schedule_table == schedules && l.by_plan;
}

static void test_names() {
    const char *const names[] = {"", "bank_stream_kernel", "bank_stream_prog_kernel", "bank_stream_bus_kernel", "bank_stream_in_kernel", "bank_stream_banks_kernel",
                                 "bank_stream_loops_kernel", "bank_stream_general_kernel"};
    const StreamKernel ks[] = {StreamKernel::none, StreamKernel::plain, StreamKernel::prog, StreamKernel::bus, StreamKernel::in, StreamKernel::banks,
                               StreamKernel::loops, StreamKernel::general};
    for (int i = 0; i < 8; ++i) {
        CHECK(std::strcmp(stream_kernel_name(ks[i]), names[i]) == 0);
        CHECK(stream_kernel_by_plan(ks[i]) == (i >= 4));
    }
}

static void test_each_kernel() {
    {   // plain: a bank that writes the rows, nothing else
        Built b;
        b.env.n_slots = 2;
        b.bank(7, false, {0, 1});
        CHECK(!stream_path(b.sp, b.list(), b.env));
        StreamBank sb;
        StreamLaunch l;
        CHECK(plain_stream_launch(2, 7, 256, sb, l));
        CHECK(l.kernel == StreamKernel::plain && one_row(l) && no_limits(l) && l.workgroups == 2 && sb.chunk_log2 == 7 && sb.voices == 2 && sb.log2_p == 7);
        CHECK(plain_stream_launch(2, 10, 256, sb, l));              // 1024 partials: chunks of 128, 8 per voice
        CHECK(l.kernel == StreamKernel::plain && one_row(l) && no_limits(l) && l.workgroups == 16 && sb.chunk_log2 == 7);
        CHECK(plain_stream_launch(2, 10, 8, sb, l) && l.workgroups == 8 && sb.chunk_log2 == 8);
        CHECK(!plain_stream_launch(9, 10, 8, sb, l));
    }
    {   // prog: a program per voice
        const Built b = kernel_plan(StreamKernel::prog);
        CHECK(stream_path(b.sp, b.list(), b.env));
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.bus_programs() == 0);
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(l.kernel == StreamKernel::prog && one_row(l) && no_limits(l) && l.workgroups == 2);
    }
    {   // bus: and a program that reads both voices of the block
        Built b = kernel_plan(StreamKernel::bus);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.bus_programs() == 1);
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(l.kernel == StreamKernel::bus && one_row(l) && no_limits(l) && l.workgroups == 2);
        b.env.bus = false;                                           // (without the option the plan is not served at all)
        CHECK(!b.plan().servable);
    }
    {   // in: a program reads slot 3 next to the time slot
        const Built b = kernel_plan(StreamKernel::in);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.input_slots == (std::vector<uint32_t>{0, 3}));
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(l.kernel == StreamKernel::in && rows_of(l, 2, false, false) && no_limits(l) && l.workgroups == 2);
    }
    {   // banks: a voice of 128 partials behind a program next to a voice of 512 that writes its row
        const Built b = kernel_plan(StreamKernel::banks);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.banks.size() == 2);
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(l.kernel == StreamKernel::banks && rows_of(l, 1, true, false) && no_limits(l) && l.workgroups == 1 + 4);
        Built c = b;                                                 // no programs, no rings: several banks alone take the program path
        c.sp = StagedPlan{};
        c.banks[0].to_ring = false;
        CHECK(stream_path(c.sp, c.list(), c.env));
        const StreamPlan t = c.plan();
        CHECK(t.servable && stream_launch(c.sp, t).kernel == StreamKernel::banks);
    }
    {   // loops: a comb of 5 frames on voice 0
        const Built b = kernel_plan(StreamKernel::loops);
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.has_loops());
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(l.kernel == StreamKernel::loops && rows_of(l, 1, true, false) && l.max_stride == 5 && l.max_loads == 2 && l.max_stores == 1 && l.workgroups == 2);
    }
    {   // general: two voices of 32 partials that write their rows
        const Built b = kernel_plan(StreamKernel::general);
        CHECK(stream_path(b.sp, b.list(), b.env));
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.has_general());
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(l.kernel == StreamKernel::general && rows_of(l, 1, true, true) && no_limits(l) && l.workgroups == 2);
    }
}

static void test_precedence() {
    // a loop program AND several banks AND control rows: loops; with a schedule bank: general
    Built b;
    b.env.n_slots = 3;
    b.env.loops = b.env.banks = b.env.inputs = b.env.bus = true;
    b.bank(7, true, {0});
    b.bank(8, false, {1});
    b.sp.feedback = true;
    b.sp.n_rings = 2;
    b.sp.input_slots = {0, 2};
    std::vector<StageInstr> p = comb(0, 1, 3);
    p.insert(p.begin() + 3, {ins(S_INPUT, 1, 0, 0, 1, 0, 0), ins(S_MUL, 0, 0, 1, 0, 0, 0)});
    b.program(p, 0, NO_RING, 0);
    b.program({ins(S_INPUT, 0, 0, 0, 1, 0, 0)}, 0, NO_RING, 2);
    {
        const StreamPlan s = b.plan();
        CHECK(s.servable && s.has_loops() && s.banks.size() == 2 && s.input_slots.size() == 2);
        const StreamLaunch l = stream_launch(b.sp, s);
        CHECK(l.kernel == StreamKernel::loops && rows_of(l, 2, true, false) && l.max_stride == 3 && l.max_loads == 3 && l.max_stores == 1 && l.workgroups == 1 + 2);
    }
    {
        Built g = b;
        g.env.general = true;
        g.env.n_slots = 4;
        g.bank(6, false, {3});
        const StreamPlan s = g.plan();
        CHECK(s.servable && s.has_loops() && s.has_general());
        const StreamLaunch l = stream_launch(g.sp, s);
        CHECK(l.kernel == StreamKernel::general && rows_of(l, 2, true, true) && l.max_stride == 3 && l.max_loads == 3 && l.max_stores == 1 && l.workgroups == 1 + 2 + 1);
    }
    {   // several banks and control rows without a loop: banks
        Built c = b;
        c.sp.instrs[c.sp.progs[0].first_instr + 1].d_lo = 100;      // the comb's own read: a block or more back
        const StreamPlan s = c.plan();
        CHECK(s.servable && !s.has_loops());
        CHECK(stream_launch(c.sp, s).kernel == StreamKernel::banks && stream_launch(c.sp, s).n_rows == 2);
    }
    {   // one bank, one slot: a bus segment decides between bus and prog, and every option being on changes nothing
        Built v = two_voices();
        v.env.bus = v.env.inputs = v.env.banks = v.env.loops = v.env.general = true;
        CHECK(stream_launch(v.sp, v.plan()).kernel == StreamKernel::prog);
        v.env.n_slots = 3;
        v.program({ins(S_READ, 0, 0, 0, 0, 0, 0), ins(S_READ, 1, 0, 0, 0, 1, 0), ins(S_SUM2, 0, 0, 1, 0, 0, 0)}, 0, NO_RING, 2);
        CHECK(v.plan().servable && stream_launch(v.sp, v.plan()).kernel == StreamKernel::bus);
    }
}

// The limits against a direct count.  The StreamPlan is hand-built: the serving rule refuses 33 loads and 17 stored rings, the
// launch rule still counts them (and the launcher refuses them).
static void test_limits() {
    for (int kind = 0; kind < 2; ++kind)
        for (uint32_t n : kind == 0 ? std::vector<uint32_t>{1, 32, 33} : std::vector<uint32_t>{1, 16, 17}) {
            std::vector<StageInstr> p{ins(S_READ, 0, 0, 0, 0, 1, 7)};               // ring 1, which the program stores: stride 7
            if (kind == 0)
                for (uint32_t i = 1; i < n; ++i) p.push_back(ins(i % 2 ? S_INPUT : S_READ, 1, 0, 0, 0, 0, 0));
            for (uint32_t r = 0; r < (kind == 1 ? n : 1u); ++r) p.push_back(ins(S_STORE, 0, 0, 0, 0, 1 + r, 0));
            p.push_back(ins(S_STORE, 0, 0, 0, 0, 1, 0));                             // (a second store of ring 1 is no second slot)
            Built b;
            b.env.n_slots = 1;
            b.env.loops = true;
            b.bank(7, true, {0});
            b.sp.feedback = true;
            b.sp.n_rings = 32;
            b.sp.input_slots = {0};
            b.program(follow(0), 0, NO_RING, 0);                                     // a program without a loop counts for nothing
            b.program(p, 0, NO_RING, -1);
            uint32_t loads = 0;
            std::set<uint32_t> stored;
            for (const StageInstr &i : p) {
                loads += i.op == S_INPUT || i.op == S_READ;
                if (i.op == S_STORE) stored.insert(i.buf);
            }
            CHECK(loads == (kind == 0 ? n : 1u) && stored.size() == (kind == 1 ? n : 1u));
            StreamPlan s;
            s.servable = true;
            s.voices = 1;
            s.banks.resize(1);
            s.banks[0].voices = 1;
            s.banks[0].log2_p = s.banks[0].chunk_log2 = 7;
            s.progs = {0, 1};
            s.loop_stride = {0, 7};
            s.voice_first = {0, 2, 2};
            const StreamLaunch l = stream_launch(b.sp, s);
            CHECK(l.kernel == StreamKernel::loops && l.max_stride == 7 && l.max_loads == loads && l.max_stores == stored.size() && l.workgroups == 1);
            const StreamPlan served = b.plan();                                      // within the tiles the serving rule agrees
            CHECK(served.servable == (loads <= STREAM_LOOP_LOADS && stored.size() <= STREAM_LOOP_STORES));
            if (served.servable) {
                const StreamLaunch m = stream_launch(b.sp, served);
                CHECK(m.kernel == StreamKernel::loops && m.max_stride == 7 && m.max_loads == loads && m.max_stores == stored.size());
            }
        }
}

// The plain path: with FR_STREAM_PROGRAMS exactly when there are no programs, no rings, one bank (or FR_STREAM_BANKS off) and no
// bank that FR_STREAM_GENERAL could serve by schedule; without the option always.
static void test_path() {
    for (int m = 0; m < 1 << 7; ++m) {
        const bool opt = m & 1, progs = m & 2, rings = m & 4, two = m & 8, env_banks = m & 16, env_general = m & 32, second_small = m & 64;
        for (int shape = 0; shape < 4; ++shape) {                                    // bank 0: 128 partials, 64, 32, a general bank
            Built b;
            b.env.programs = opt;
            b.env.banks = env_banks;
            b.env.general = env_general;
            b.env.bus = b.env.inputs = b.env.loops = true;                           // (these never decide the path)
            b.bank(shape == 1 ? 6 : shape == 2 ? 5 : 7, false, {0});
            b.banks[0].general = shape == 3;
            if (two) b.bank(second_small ? 6 : 9, false, {1});
            if (progs) b.program({ins(S_CONST, 0, 0, 0, 0, 0, 0)}, 0, NO_RING, 2);
            if (rings) b.sp.n_rings = 1;
            const bool schedulable = shape != 0 || (two && second_small);
            const bool plain = !opt || (!progs && !rings && !(env_banks && two) && !(env_general && schedulable));
            CHECK(stream_path(b.sp, b.list(), b.env) == !plain);
        }
    }
}

// One-bank dealing: the loop fr_stream_begin had, restated, against deal_stream_chunks through plain_stream_launch.
static void test_dealing() {
    for (uint32_t voices = 1; voices <= 256; ++voices)
        for (uint32_t log2_p = 7; log2_p <= 15; ++log2_p)
            for (uint64_t max_wgs : {1ull, 8ull, 32ull, 64ull, 255ull, 256ull}) {
                uint32_t c = log2_p;
                while (c > 7 && ((uint64_t)voices << (log2_p - c + 1)) <= max_wgs && log2_p - c < 8) --c;
                const bool refused = ((uint64_t)voices << (log2_p - c)) > max_wgs;
                StreamBank sb;
                StreamLaunch l;
                const bool ok = plain_stream_launch(voices, log2_p, max_wgs, sb, l);
                if (ok == refused || (ok && (sb.chunk_log2 != c || l.workgroups != voices << (log2_p - c) || sb.first_wg != 0 || sb.first_voice != 0))) {
                    ++failed;
                    std::printf("FAILED dealing: %u voices, log2_p %u, max_wgs %llu: old chunk_log2 %u refused %d, new %u refused %d\n", voices, log2_p,
                                (unsigned long long)max_wgs, c, (int)refused, sb.chunk_log2, (int)!ok);
                } else {
                    ++passed;
                }
            }
}

int main() {
    test_names();
    test_each_kernel();
    test_precedence();
    test_limits();
    test_path();
    test_dealing();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
