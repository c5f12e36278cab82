// streamcheck_tests.cpp -- what a resident launch checks before it launches (libfriendship_amd/csrc/kernels.hpp
// stream_launch_check, the host logic of kernels.hip launch_bank_stream): for each of the eight kernels a minimal accepted
// argument set and its workgroup count, then every checked field broken one at a time and the refusal; what a kernel's form
// does not read is accepted whatever it holds.  And the form the check assumes per kernel (StreamForm) against the launch
// rule's record (streamplan.hpp StreamLaunch) on the hand-built plans of streamplans.hpp.  Stand-alone: built and run on the
// CPU with -fsanitize=address,undefined by tests/test_stream_check_host.py.
#include <functional>
#include <string>
#include <vector>

#include "streamplans.hpp"

static const StreamKernel KERNELS[] = {StreamKernel::plain, StreamKernel::prog,  StreamKernel::bus,     StreamKernel::in,
                                       StreamKernel::banks, StreamKernel::loops, StreamKernel::general, StreamKernel::dyn};

// Something for every pointer to point at: the check reads none of it.
static float2 some_params[1];
static float some_floats[1];
static uint32_t some_words[4];
static StageInstr some_instrs[1];
static StageProg some_progs[1];
static BankStreamInCtl some_ctl;
static BankStreamInDev some_dev;

// The minimal accepted arguments of kernel `k`: one voice of 128 partials in one chunk; with a bank table (1 voice, 128
// partials) and (1 voice, 512 partials in chunks of 128); with schedule banks also one of one voice.  Everything is filled in
// for every kernel: what a form does not take is there to be ignored.
static StreamLaunchArgs minimal(StreamKernel k) {
    const StreamForm f = stream_form(k);
    StreamLaunchArgs x{};
    x.a.params = some_params;
    x.a.out = some_floats;
    x.a.rows = some_words;
    x.a.n_voices = f.schedule ? 3 : f.table ? 2 : 1;
    x.a.log2_p = x.a.chunk_log2 = 7;
    x.a.leaf_variant = 1;
    x.a.ws = some_floats;
    x.a.tickets = some_words;
    x.p.instrs = some_instrs;
    x.p.progs = some_progs;
    x.p.voice_first = some_words;
    x.p.rings = some_floats;
    x.p.ring_mask = 63;
    x.p.n_rings = 1;
    x.p.bank_to_ring = 1;
    x.t.n_banks = f.schedule ? 3 : 2;
    x.t.bank[0] = {some_params, some_words, 0, 0, 1, 7, 7, 1, 1};
    x.t.bank[1] = {some_params, some_words, 1, 1, 1, 9, 7, 1, 0};
    x.t.bank[2] = {some_params, some_words, 5, 2, 1, 0, 0, 1, 0};   // the schedule bank: its log2_p and chunk_log2 are not read
    x.g.mask = 1u << 2;
    x.g.bank[2].groups = x.g.bank[2].group_off = some_words;
    x.n_rows = 1;
    x.max_stride = 5; x.max_loads = 2; x.max_stores = 1;
    x.ctl_dev = &some_ctl;
    x.dev = &some_dev;
    return x;
}
static uint32_t minimal_wgs(StreamKernel k) { return stream_form(k).schedule ? 6 : stream_form(k).table ? 5 : 1; }

// One broken field: the forms it is checked in (all others must go on accepting it), what it does to the arguments.
struct Break {
    const char *what;
    std::function<bool(const StreamForm &)> checked;
    std::function<void(StreamLaunchArgs &)> apply;
};
static bool any(const StreamForm &) { return true; }
static bool one_bank(const StreamForm &f) { return !f.table; }
static bool progs(const StreamForm &f) { return f.progs; }
static bool rows(const StreamForm &f) { return f.rows; }
static bool table(const StreamForm &f) { return f.table; }
static bool loops(const StreamForm &f) { return f.loops; }
static bool loops_only(const StreamForm &f) { return f.loops && !f.schedule; }
static bool schedule(const StreamForm &f) { return f.schedule; }
static bool general_only(const StreamForm &f) { return f.schedule && !f.dyn; }
static void no_ring_feeds(StreamLaunchArgs &x) {   // (so that a plan without rings passes stream_progs_ok)
    x.p.bank_to_ring = 0;
    x.t.bank[0].to_ring = 0;
}

static const std::vector<Break> BREAKS = {
    // every kernel
    {"leaf_variant 0", any, [](StreamLaunchArgs &x) { x.a.leaf_variant = 0; }},
    {"leaf_variant 2", any, [](StreamLaunchArgs &x) { x.a.leaf_variant = 2; }},
    {"out null", any, [](StreamLaunchArgs &x) { x.a.out = nullptr; }},
    {"ctl null", any, [](StreamLaunchArgs &x) { x.ctl_dev = nullptr; }},
    {"dev null", any, [](StreamLaunchArgs &x) { x.dev = nullptr; }},
    // the one bank of BankArgs (stream_bank_ok).  With a table BankArgs' n_voices must be the table's voices, and its ws and
    // tickets serve the table's chunked bank: broken for every kernel
    {"rows null", one_bank, [](StreamLaunchArgs &x) { x.a.rows = nullptr; }},
    {"chunk_log2 6", one_bank, [](StreamLaunchArgs &x) { x.a.chunk_log2 = 6; }},
    {"chunk_log2 14", one_bank, [](StreamLaunchArgs &x) { x.a.log2_p = x.a.chunk_log2 = 14; }},
    {"chunk_log2 > log2_p", one_bank, [](StreamLaunchArgs &x) { x.a.log2_p = 6; }},
    {"512 chunks", one_bank, [](StreamLaunchArgs &x) { x.a.log2_p = 16; }},
    {"no voices", any, [](StreamLaunchArgs &x) { x.a.n_voices = 0; }},
    {"257 workgroups", any, [](StreamLaunchArgs &x) { x.a.n_voices = 257; }},
    {"258 workgroups", any, [](StreamLaunchArgs &x) { x.a.n_voices = 129; x.a.log2_p = 8; }},
    {"2^32 + 2 workgroups", any, [](StreamLaunchArgs &x) { x.a.n_voices = 0x80000001u; x.a.log2_p = 8; }},
    {"chunks without ws", any, [](StreamLaunchArgs &x) { x.a.log2_p = 8; x.a.ws = nullptr; }},
    {"chunks without tickets", any, [](StreamLaunchArgs &x) { x.a.log2_p = 8; x.a.tickets = nullptr; }},
    // the programs' arguments (stream_progs_ok)
    {"voice_first null", progs, [](StreamLaunchArgs &x) { x.p.voice_first = nullptr; }},
    {"ring_mask 62", progs, [](StreamLaunchArgs &x) { x.p.ring_mask = 62; }},
    {"rings null", progs, [](StreamLaunchArgs &x) { x.p.rings = nullptr; }},
    {"rings of 32 frames", progs, [](StreamLaunchArgs &x) { x.p.ring_mask = 31; }},
    {"a bank feeds rings, no rings", progs, [](StreamLaunchArgs &x) { x.p.n_rings = 0; x.max_stride = 0; }},
    // the doorbell of rows
    {"n_rows 0", rows, [](StreamLaunchArgs &x) { x.n_rows = 0; }},
    {"n_rows 9", rows, [](StreamLaunchArgs &x) { x.n_rows = BANK_STREAM_ROWS + 1; }},
    // the bank table (stream_table_ok)
    {"n_banks 0", table, [](StreamLaunchArgs &x) { x.t.n_banks = 0; }},
    {"n_banks 9", table, [](StreamLaunchArgs &x) { x.t.n_banks = BANK_STREAM_BANKS + 1; }},
    {"bank chunk_log2 6", table, [](StreamLaunchArgs &x) { x.t.bank[1].chunk_log2 = 6; }},
    {"bank chunk_log2 14", table, [](StreamLaunchArgs &x) { x.t.bank[0].log2_p = x.t.bank[0].chunk_log2 = 14; }},
    {"bank chunk_log2 > log2_p", table, [](StreamLaunchArgs &x) { x.t.bank[0].log2_p = 6; }},
    {"bank of 512 chunks", table, [](StreamLaunchArgs &x) { x.t.bank[1].log2_p = 16; }},
    {"bank without voices", table, [](StreamLaunchArgs &x) { x.t.bank[0].n_voices = 0; }},
    {"bank of 257 workgroups", table, [](StreamLaunchArgs &x) { x.t.bank[0].n_voices = 257; }},
    {"bank params null", table, [](StreamLaunchArgs &x) { x.t.bank[1].params = nullptr; }},
    {"bank rows null", table, [](StreamLaunchArgs &x) { x.t.bank[1].rows = nullptr; }},
    {"first_wg leaves a gap", table, [](StreamLaunchArgs &x) { x.t.bank[1].first_wg = 2; }},
    {"first_wg overlaps", table, [](StreamLaunchArgs &x) { x.t.bank[1].first_wg = 0; }},
    {"first_voice leaves a gap", table, [](StreamLaunchArgs &x) { x.t.bank[1].first_voice = 2; }},
    {"voices of the table != n_voices", table, [](StreamLaunchArgs &x) { x.t.bank[x.t.n_banks - 1].n_voices += 1; }},
    // the loop programs' tiles
    {"max_stride 64", loops, [](StreamLaunchArgs &x) { x.max_stride = BANK_STREAM_LOOP_MAX_STRIDE + 1; }},
    {"max_loads 33", loops, [](StreamLaunchArgs &x) { x.max_loads = BANK_STREAM_LOOP_LOADS + 1; }},
    {"max_stores 17", loops, [](StreamLaunchArgs &x) { x.max_stores = BANK_STREAM_LOOP_STORES + 1; }},
    {"a loop, no rings", loops, [](StreamLaunchArgs &x) { no_ring_feeds(x); x.p.n_rings = 0; }},
    {"the loops kernel, no rings", loops_only, [](StreamLaunchArgs &x) { no_ring_feeds(x); x.p.n_rings = 0; x.max_stride = 0; }},
    // the schedule banks
    {"no schedule bank", general_only, [](StreamLaunchArgs &x) { x.g.mask = 0; x.t.bank[2].log2_p = x.t.bank[2].chunk_log2 = 7; }},
    {"mask beyond the table", schedule, [](StreamLaunchArgs &x) { x.g.mask |= 1u << 3; }},
    {"groups null", schedule, [](StreamLaunchArgs &x) { x.g.bank[2].groups = nullptr; }},
    {"group_off null", schedule, [](StreamLaunchArgs &x) { x.g.bank[2].group_off = nullptr; }},
    {"schedule bank without voices", schedule, [](StreamLaunchArgs &x) { x.t.bank[2].n_voices = 0; }},
    {"schedule bank params null", schedule, [](StreamLaunchArgs &x) { x.t.bank[2].params = nullptr; }},
    {"schedule bank rows null", schedule, [](StreamLaunchArgs &x) { x.t.bank[2].rows = nullptr; }},
    {"schedule bank first_wg", schedule, [](StreamLaunchArgs &x) { x.t.bank[2].first_wg = 4; }},
};

static void test_minimal_and_breaks() {
    for (StreamKernel k : KERNELS) {
        const StreamForm f = stream_form(k);
        const uint32_t wgs = minimal_wgs(k);
        CHECK(stream_launch_check(k, minimal(k)) == wgs);
        for (const Break &b : BREAKS) {
            StreamLaunchArgs x = minimal(k);
            b.apply(x);
            const uint32_t got = stream_launch_check(k, x);
            // (a break of a field the form does not take changes nothing)
            const uint32_t want = b.checked(f) ? 0u : wgs;
            if (got != want) {
                ++failed;
                std::printf("FAILED %s, %s: %u workgroups, expected %u\n", stream_kernel_name(k), b.what, got, want);
            } else {
                ++passed;
            }
        }
        CHECK(stream_launch_check(StreamKernel::none, minimal(k)) == 0);
        CHECK(stream_launch_check((StreamKernel)((uint32_t)StreamKernel::dyn + 1), minimal(k)) == 0);
        CHECK(stream_launch_check((StreamKernel)0xFFFFFFFFu, minimal(k)) == 0);
    }
}

// The edges that are accepted, and the workgroup counts of larger launches.
static void test_accepted() {
    for (StreamKernel k : KERNELS) {
        const StreamForm f = stream_form(k);
        StreamLaunchArgs x = minimal(k);
        if (!f.table) {
            x.a.n_voices = 256;                                      // the residency bound itself
            CHECK(stream_launch_check(k, x) == 256);
            x.a.n_voices = 1; x.a.log2_p = 15;                       // 256 chunks of 128
            CHECK(stream_launch_check(k, x) == 256);
            x.a.log2_p = x.a.chunk_log2 = 13;                        // the largest chunk; one chunk needs no workspace
            x.a.ws = nullptr; x.a.tickets = nullptr;
            CHECK(stream_launch_check(k, x) == 1);
            x.a.n_voices = 3; x.a.log2_p = 10; x.a.chunk_log2 = 8; x.a.ws = some_floats; x.a.tickets = some_words;
            CHECK(stream_launch_check(k, x) == 12);
        } else {
            x.a.rows = nullptr;                                      // (a table kernel reads the banks' rows, not BankArgs')
            x.a.log2_p = x.a.chunk_log2 = 0;
            CHECK(stream_launch_check(k, x) == minimal_wgs(k));
            x.t.bank[1].n_voices = 63;                               // 1 + 63 * 4 (+ 1) workgroups: 254 voices' worth below the bound
            x.t.bank[2].first_wg = 253; x.t.bank[2].first_voice = 64; x.a.n_voices += 62;
            CHECK(stream_launch_check(k, x) == (f.schedule ? 254u : 253u));
            x.t.bank[1].n_voices = 64;                               // 1 + 64 * 4: one bank within the bound, the launch beyond it
            x.t.bank[2].first_wg = 257; x.t.bank[2].first_voice = 65; x.a.n_voices += 1;
            CHECK(stream_launch_check(k, x) == 0);
        }
        if (f.rows) {
            x = minimal(k);
            x.n_rows = BANK_STREAM_ROWS;
            CHECK(stream_launch_check(k, x) == minimal_wgs(k));
        }
        if (f.loops) {
            x = minimal(k);
            x.max_stride = BANK_STREAM_LOOP_MAX_STRIDE; x.max_loads = BANK_STREAM_LOOP_LOADS; x.max_stores = BANK_STREAM_LOOP_STORES;
            CHECK(stream_launch_check(k, x) == minimal_wgs(k));
        }
        if (f.progs) {                                               // no rings at all: fine where no bank feeds one
            x = minimal(k);
            no_ring_feeds(x);
            x.p.n_rings = 0; x.p.rings = nullptr; x.p.ring_mask = 0; x.max_stride = 0;
            CHECK(stream_launch_check(k, x) == (f.loops && !f.schedule ? 0u : minimal_wgs(k)));
        }
    }
    {   // dyn alone takes a plan without a schedule bank: the third bank a balanced one
        StreamLaunchArgs x = minimal(StreamKernel::dyn);
        x.g = StreamGeneralArgs{};
        x.t.bank[2].log2_p = x.t.bank[2].chunk_log2 = 7;
        CHECK(stream_launch_check(StreamKernel::dyn, x) == 6);
        CHECK(stream_launch_check(StreamKernel::general, x) == 0);
    }
}

// The form per kernel: a cascade, and what the launch rule's record says of the same kernel.
static void test_form() {
    for (StreamKernel k : KERNELS) {
        const StreamForm f = stream_form(k);
        CHECK((uint32_t)f.progs + f.bus + f.rows + f.table + f.loops + f.schedule + f.dyn == (uint32_t)k - (uint32_t)StreamKernel::plain);
        CHECK(f.progs >= f.bus && f.bus >= f.rows && f.rows >= f.table && f.table >= f.loops && f.loops >= f.schedule && f.schedule >= f.dyn);
        StreamLaunch l;
        if (k == StreamKernel::plain) {
            StreamBank sb;
            CHECK(plain_stream_launch(2, 7, 256, sb, l));
        } else {
            const Built b = kernel_plan(k);
            const StreamPlan s = b.plan();
            CHECK(s.servable);
            l = stream_launch(b.sp, s);
        }
        CHECK(l.kernel == k);
        CHECK(f.rows == l.rows_doorbell && f.table == l.bank_table);
        CHECK(l.schedule_table ? f.schedule : !f.schedule || f.dyn);   // (dyn takes the schedule table only with schedule banks)
        CHECK(f.rows || l.n_rows == 1);
    }
    static_assert(!stream_form(StreamKernel::plain).progs && stream_form(StreamKernel::prog).progs && !stream_form(StreamKernel::prog).bus, "");
    static_assert(stream_form(StreamKernel::in).rows && !stream_form(StreamKernel::bus).rows && stream_form(StreamKernel::dyn).schedule, "");
}

int main() {
    test_minimal_and_breaks();
    test_accepted();
    test_form();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
