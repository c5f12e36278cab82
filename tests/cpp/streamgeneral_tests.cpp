// streamgeneral_tests.cpp -- FR_STREAM_GENERAL on the host (libfriendship_amd/csrc/streamplan.hpp): the schedule validation on
// well-formed schedules and on each malformed kind, the one-item schedules of balanced 32- and 64-partial banks, the chunk
// dealing with schedule banks mixed in, the serving rule on hand-built banks, and a plain-loop model of the kernel's schedule
// renderer (kernels.hip stream_render_schedule: 16 "waves", the ladder, the double-buffered hand-over, the stack) on random leaf
// values against a direct evaluation of the tree the schedule describes, bit for bit.  Stand-alone: built and run on the CPU with
// -fsanitize=address,undefined by tests/test_stream_general_host.py.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
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

static uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

// ---- a Sum2 tree over leaves, and the schedule the matcher makes of it (match.cpp emit_general) -------------------------
struct Tree {
    int k = -1;                        // >= 0: a complete sub-tree of 2^k leaves (an item)
    std::unique_ptr<Tree> a, b;        // else: a + b
};
static std::unique_ptr<Tree> item(int k) { auto t = std::make_unique<Tree>(); t->k = k; return t; }
static std::unique_ptr<Tree> sum(std::unique_ptr<Tree> a, std::unique_ptr<Tree> b) {
    auto t = std::make_unique<Tree>();
    t->a = std::move(a); t->b = std::move(b);
    return t;
}
// post-order: an item is a word, every other node a merge after its right operand
static void emit(const Tree &t, std::vector<uint32_t> &groups) {
    if (t.k >= 0) { groups.push_back((uint32_t)t.k); return; }
    emit(*t.a, groups);
    emit(*t.b, groups);
    groups.back() += 1u << 4;
}
static uint32_t leaves_of(const Tree &t) { return t.k >= 0 ? 1u << t.k : leaves_of(*t.a) + leaves_of(*t.b); }

// the tree itself: a complete sub-tree adds its halves, a node adds its operands, left on the left
static float eval_complete(const float *leaf, uint32_t n) { return n == 1 ? leaf[0] : eval_complete(leaf, n / 2) + eval_complete(leaf + n / 2, n / 2); }
static float eval(const Tree &t, const float *&leaf) {
    if (t.k >= 0) {
        const float v = eval_complete(leaf, 1u << t.k);
        leaf += 1u << t.k;
        return v;
    }
    const float a = eval(*t.a, leaf);
    const float b = eval(*t.b, leaf);
    return a + b;
}

// ---- the kernel's schedule renderer, one frame, as plain loops ------------------------------------------------------------
// `pairs`: the voice's leaf VALUES where the kernel has {w, A} pairs: item after item, an item of fewer than 8 leaves padded to
// 8 (padding is poisoned with NaN: it is never a leaf).
static float group_sum(const float *l) { return ((l[0] + l[1]) + (l[2] + l[3])) + ((l[4] + l[5]) + (l[6] + l[7])); }
static float small_group(const float *l, uint32_t j) {   // gbank_group
    float v = l[0];
    if (j >= 1) {
        v = l[0] + l[1];
        if (j >= 2) {
            v = v + (l[2] + l[3]);
            if (j >= 3) v = v + ((l[4] + l[5]) + (l[6] + l[7]));
        }
    }
    return v;
}
static float wave_sum(const float *l, uint32_t ngroups, uint32_t levels) {   // bank_wave_sum: the binary-counter carry over groups of 8
    float s[9] = {0};
    for (uint32_t g = 0; g < ngroups; ++g) {
        float v = group_sum(l + (size_t)g * 8);
        uint32_t lvl = 0;
        while (lvl < 8 && ((g >> lvl) & 1u)) { v = s[lvl] + v; ++lvl; }
        s[lvl] = v;
    }
    return s[levels];
}
static bool model(const std::vector<uint32_t> &groups, const std::vector<float> &pairs, float &root, uint32_t &barriers) {
    constexpr uint32_t NW = 16;
    float sm[2][NW];
    for (auto &b : sm) for (float &x : b) x = std::nanf("");      // whatever LDS held
    float stack[STREAM_SCHEDULE_MAX_DEPTH];
    uint32_t sp = 0, goff = 0, nbig = 0;
    barriers = 0;
    auto finish = [&](float v, uint32_t meta) {
        for (uint32_t m = meta >> 4; m != 0; --m) {
            if (sp == 0) return false;
            --sp;
            v = stack[sp] + v;
        }
        if (sp >= STREAM_SCHEDULE_MAX_DEPTH) return false;
        stack[sp++] = v;
        return true;
    };
    for (uint32_t meta : groups) {
        const uint32_t k = meta & 15u;
        if (k >= 4) {
            const uint32_t wl = k >= 7 ? 4 : k - 3, lv = k - 3 - wl;
            float *buf = sm[nbig++ & 1u];
            for (uint32_t wave = 0; wave < NW; ++wave)
                if (wave < (1u << wl)) buf[wave] = wave_sum(pairs.data() + ((size_t)goff + ((size_t)wave << lv)) * 8, 1u << lv, lv);
            ++barriers;
            float s[NW];
            for (uint32_t j = 0; j < NW; ++j) s[j] = buf[j];
            float rung[5];
            rung[0] = s[0];
            for (uint32_t level = 1, n = NW / 2; level <= 4; ++level, n /= 2) {
                for (uint32_t j = 0; j < n; ++j) s[j] = s[2 * j] + s[2 * j + 1];
                rung[level] = s[0];
            }
            if (!finish(rung[wl], meta)) return false;
            goff += 1u << (k - 3);
        } else {
            if (!finish(small_group(pairs.data() + (size_t)goff * 8, k), meta)) return false;
            goff += 1;
        }
    }
    if (sp != 1) return false;
    root = stack[0];
    return true;
}

static void run_tree(const Tree &t, std::mt19937 &rng, const char *what) {
    std::vector<uint32_t> groups;
    emit(t, groups);
    const std::vector<uint32_t> group_off{0, 0, (uint32_t)groups.size(), 0};
    std::string why;
    const bool ok = stream_schedule_ok(groups, group_off, 0, &why);
    CHECK(ok);
    if (!ok) { std::printf("  %s: %s\n", what, why.c_str()); return; }
    CHECK(stream_schedule_leaves(groups, group_off, 0) == leaves_of(t));
    const uint32_t n = leaves_of(t);
    std::uniform_real_distribution<float> mant(-1.0f, 1.0f);
    std::uniform_int_distribution<int> expo(-12, 12);
    uint32_t expected_barriers = 0;
    for (uint32_t g : groups) expected_barriers += (g & 15u) >= 4 ? 1 : 0;
    for (int round = 0; round < 4; ++round) {
        std::vector<float> leaf(n), pairs;
        for (float &x : leaf) x = std::ldexp(mant(rng), expo(rng));   // magnitudes apart: every association rounds differently
        if (round == 3) for (float &x : leaf) x = -0.0f;               // a silent voice: the root is -0
        size_t at = 0;
        for (uint32_t g : groups) {
            const uint32_t sz = 1u << (g & 15u);
            pairs.insert(pairs.end(), leaf.begin() + at, leaf.begin() + at + sz);
            if (sz < 8) pairs.resize(pairs.size() + 8 - sz, std::nanf(""));
            at += sz;
        }
        CHECK(pairs.size() == stream_schedule_pairs(groups, group_off, 0));
        const float *lp = leaf.data();
        const float want = eval(t, lp);
        CHECK(lp == leaf.data() + n);
        float got = 0;
        uint32_t barriers = 0;
        CHECK(model(groups, pairs, got, barriers));
        CHECK(barriers == expected_barriers);
        if (bits(got) != bits(want)) std::printf("  %s round %d: got %a want %a\n", what, round, got, want);
        CHECK(bits(got) == bits(want));
    }
}

static std::unique_ptr<Tree> balanced(uint32_t n) {   // synth.sum_tree: adjacent pairs level by level, an odd one carried up
    std::vector<std::unique_ptr<Tree>> cur;
    for (uint32_t i = 0; i < n; ++i) cur.push_back(item(0));
    while (cur.size() > 1) {
        std::vector<std::unique_ptr<Tree>> next;
        for (size_t i = 0; i + 1 < cur.size(); i += 2) next.push_back(sum(std::move(cur[i]), std::move(cur[i + 1])));
        if (cur.size() % 2) next.push_back(std::move(cur.back()));
        cur = std::move(next);
    }
    return std::move(cur[0]);
}
// the matcher's cut: maximal complete sub-trees of at most 2048 leaves become items
static int complete(Tree &t) {
    if (t.k >= 0) return t.k;
    const int a = complete(*t.a), b = complete(*t.b);
    if (a >= 0 && a == b && a < 11) { t.k = a + 1; t.a.reset(); t.b.reset(); return t.k; }
    return -1;
}
static std::unique_ptr<Tree> random_tree(std::mt19937 &rng, uint32_t depth) {
    if (depth == 0 || rng() % 3 == 0) return item((int)(rng() % 12));
    return sum(random_tree(rng, depth - 1), random_tree(rng, depth - 1));
}

static void test_model() {
    std::mt19937 rng(0x5EED0900);
    for (int k = 0; k <= 11; ++k) {                       // every item size alone, and as either operand of a merge
        run_tree(*item(k), rng, "one item");
        run_tree(*sum(item(k), item(0)), rng, "item + leaf");
        run_tree(*sum(item(1), item(k)), rng, "pair + item");
        run_tree(*sum(sum(item(k), item(2)), sum(item(11 - k), item(k))), rng, "two merges");
    }
    for (uint32_t n : {16u, 24u, 100u, 129u, 300u, 1000u, 3000u}) {   // the voices of synth.additive_tree
        auto t = balanced(n);
        complete(*t);
        run_tree(*t, rng, "additive voice");
        std::vector<uint32_t> g;
        emit(*t, g);
        if (n == 24) CHECK(g == (std::vector<uint32_t>{4, 3 | 1u << 4}));
        if (n == 100) CHECK(g == (std::vector<uint32_t>{6, 5, 2 | 2u << 4}));          // 64 + (32 + 4): the odd one is carried up
        if (n == 129) CHECK(g == (std::vector<uint32_t>{7, 0 | 1u << 4}));
        if (n == 1000) CHECK(g.size() == 6 && stream_schedule_leaves(g, {0, 0, 6, 0}, 0) == 1000);   // 512 + 256 + 128 + 64 + 32 + 8
    }
    {   // a left chain of 20 leaves; a balanced 128-leaf sub-tree plus a 3-leaf one, and its mirror
        auto chain = item(0);
        for (int i = 1; i < 20; ++i) chain = sum(std::move(chain), item(0));
        complete(*chain);
        run_tree(*chain, rng, "left chain");
        run_tree(*sum(item(7), sum(item(1), item(0))), rng, "128 + 3");
        run_tree(*sum(sum(item(1), item(0)), item(7)), rng, "3 + 128");
    }
    {   // a right chain reaches the deepest stack the kernel has: 16 pending operands
        auto chain = item(4);
        for (int i = 1; i < 16; ++i) chain = sum(item(i % 12), std::move(chain));
        run_tree(*chain, rng, "right chain of 16");
    }
    for (int i = 0; i < 60; ++i) {
        auto t = random_tree(rng, 4);
        run_tree(*t, rng, "random tree");
    }
}

static void test_schedule_ok() {
    std::string why;
    auto ok = [&](std::vector<uint32_t> g) { return stream_schedule_ok(g, {0, 0, (uint32_t)g.size(), 0}, 0, &why); };
    CHECK(ok({4}));
    CHECK(ok({6, 5 | 1u << 4, 2 | 1u << 4}));
    CHECK(ok({0, 0, 0 | 2u << 4}));
    CHECK(ok({11, 11 | 1u << 4}));
    CHECK(!ok({3 | 1u << 4}) && why.find("underflows") != std::string::npos);                 // a merge with nothing below
    CHECK(!ok({3, 3 | 2u << 4}) && why.find("underflows") != std::string::npos);
    CHECK(!ok(std::vector<uint32_t>(17, 0)) && why.find("deeper than 16") != std::string::npos);   // depth 17
    {
        std::vector<uint32_t> g(16, 0);                                                       // depth 16 is what the stack holds
        g.back() |= 15u << 4;
        CHECK(ok(g));
    }
    CHECK(!ok({3, 3}) && why.find("leaves 2 values") != std::string::npos);                   // two values left
    CHECK(!ok({12}) && why.find("2048") != std::string::npos);                                // k = 12
    CHECK(!ok({}) && why.find("empty") != std::string::npos);                                 // an empty voice
    // voices of a bank: the second one's words only
    const std::vector<uint32_t> groups{4, 3 | 1u << 4, 5, 12};
    const std::vector<uint32_t> off{0, 0, 2, 3, 3, 7, 4, 8};
    CHECK(stream_schedule_ok(groups, off, 0) && stream_schedule_ok(groups, off, 1) && !stream_schedule_ok(groups, off, 2));
    CHECK(!stream_schedule_ok(groups, off, 3));                                               // no such voice
    CHECK(!stream_schedule_ok(groups, {0, 0, 9, 0}, 0));                                      // items beyond the words
    CHECK(stream_schedule_leaves(groups, off, 0) == 24 && stream_schedule_leaves(groups, off, 1) == 32);
    CHECK(stream_schedule_pairs(groups, off, 0) == 24 && stream_schedule_pairs({2, 0 | 1u << 4}, {0, 0, 2, 2}, 0) == 16);
}

static void test_balanced_schedules() {
    for (uint32_t log2_p : {5u, 6u}) {
        std::vector<uint32_t> groups, off;
        stream_balanced_schedule(3, log2_p, groups, off);
        CHECK(groups == std::vector<uint32_t>(3, log2_p) && off.size() == 8);
        for (uint32_t v = 0; v < 3; ++v) {
            CHECK(stream_schedule_ok(groups, off, v));
            CHECK(off[2 * v] == v && off[2 * v + 2] == v + 1);
            CHECK((uint64_t)off[2 * v + 1] * 8 == (uint64_t)v << log2_p);                     // where [voices][P] pairs have voice v
            CHECK(stream_schedule_leaves(groups, off, v) == 1u << log2_p && stream_schedule_pairs(groups, off, v) == 1u << log2_p);
        }
        CHECK(!stream_schedule_ok(groups, off, 3));
    }
}

static StreamBank bank(uint32_t voices, uint32_t log2_p, bool general = false) {
    StreamBank b;
    b.voices = voices;
    b.log2_p = log2_p;
    b.general = general;
    return b;
}

static void test_deal() {
    {   // a schedule bank alone: one workgroup per voice, never halved, whatever its log2_p says
        std::vector<StreamBank> b{bank(24, 0, true)};
        CHECK(deal_stream_chunks(b, 256) && b[0].chunk_log2 == 0 && b[0].first_wg == 0);
        std::vector<StreamBank> c{bank(257, 0, true)};
        CHECK(!deal_stream_chunks(c, 256));
        std::vector<StreamBank> d{bank(2, 6, true)};
        CHECK(deal_stream_chunks(d, 256) && d[0].chunk_log2 == 6);
    }
    {   // mixed: the chunked banks share what the schedule voices leave
        std::vector<StreamBank> b{bank(1, 8), bank(2, 0, true), bank(2, 6, true)};
        CHECK(deal_stream_chunks(b, 256));
        CHECK(b[0].chunk_log2 == 7 && b[1].chunk_log2 == 0 && b[2].chunk_log2 == 6);
        CHECK(b[0].first_wg == 0 && b[1].first_wg == 2 && b[2].first_wg == 4 && b[1].first_voice == 1 && b[2].first_voice == 3);
        std::vector<StreamBank> with{bank(4, 13), bank(100, 0, true)}, without{bank(4, 13)};
        CHECK(deal_stream_chunks(with, 256) && deal_stream_chunks(without, 156));
        CHECK(with[0].chunk_log2 == without[0].chunk_log2 && with[1].first_wg == (4u << (13 - with[0].chunk_log2)));
        CHECK((4u << (13 - with[0].chunk_log2)) + 100 <= 256);
        std::vector<StreamBank> full{bank(200, 7), bank(57, 0, true)};
        CHECK(!deal_stream_chunks(full, 256));
        full[1].voices = 56;
        CHECK(deal_stream_chunks(full, 256));
    }
    {   // a `general` flag that is false changes nothing (tests/cpp/streambanks_tests.cpp is the rule's own test)
        std::vector<StreamBank> a{bank(2, 10), bank(3, 8), bank(4, 7)}, b = a;
        for (StreamBank &x : b) x.general = false;
        CHECK(deal_stream_chunks(a, 256) && deal_stream_chunks(b, 256));
        for (size_t i = 0; i < a.size(); ++i) CHECK(a[i].chunk_log2 == b[i].chunk_log2 && a[i].first_wg == b[i].first_wg);
    }
}

// ---- the rule on hand-built banks ------------------------------------------------------------------------------------
static BankLaunch general_bank(const std::vector<std::vector<uint32_t>> &voices, uint32_t first_row = 0) {
    BankLaunch b;
    b.general = true;
    b.group_off = {0, 0};
    for (const std::vector<uint32_t> &g : voices) {
        b.rows.push_back(first_row + (uint32_t)b.rows.size());
        b.groups.insert(b.groups.end(), g.begin(), g.end());
        uint32_t pairs = 0;
        for (uint32_t w : g) pairs += std::max(8u, 1u << (w & 15u));
        b.params.resize(b.params.size() + 2 * (size_t)pairs, 0.0f);
        b.group_off.push_back((uint32_t)b.groups.size());
        b.group_off.push_back((uint32_t)(b.params.size() / 16));
    }
    return b;
}
static BankLaunch balanced_bank(uint32_t voices, uint32_t log2_p, uint32_t first_row) {
    BankLaunch b;
    b.log2_p = log2_p;
    for (uint32_t v = 0; v < voices; ++v) b.rows.push_back(first_row + v);
    b.params.resize(((size_t)voices << log2_p) * 2, 0.0f);
    return b;
}
static StreamPlan rule(const std::vector<const BankLaunch *> &banks, uint32_t n_slots, bool general, bool several = false) {
    StagedPlan sp;
    StreamEnv env;
    env.n_slots = n_slots;
    env.general = general;
    env.banks = several;
    return plan_stream(sp, banks, env);
}

static void test_rule() {
    const BankLaunch g = general_bank({{6, 5 | 1u << 4, 2 | 1u << 4}, {4, 3 | 1u << 4}});
    {
        const StreamPlan off = rule({&g}, 2, false);
        CHECK(!off.servable && off.reason == "block streaming needs balanced template voices (these are general, compiled or track voices)");
        CHECK(off.general_voices.empty() && off.banks.empty());
        const StreamPlan on = rule({&g}, 2, true);
        CHECK(on.servable && on.has_general() && on.general_voices == (std::vector<uint32_t>{100, 24}));
        CHECK(on.voices == 2 && on.chunks == 1 && on.workgroups() == 2 && on.banks.size() == 1 && on.banks[0].general && on.banks[0].max_leaves == 100);
        CHECK(on.programs_per_voice() == (std::vector<uint32_t>{0, 0}) && on.bus_programs() == 0);
    }
    for (uint32_t log2_p : {5u, 6u}) {
        const BankLaunch b = balanced_bank(2, log2_p, 0);
        const StreamPlan off = rule({&b}, 2, false);
        CHECK(!off.servable && off.reason == "block streaming needs voices of at least 128 partials (16 waves x one group of 8)");
        const StreamPlan on = rule({&b}, 2, true);
        CHECK(on.servable && on.has_general() && on.general_voices == std::vector<uint32_t>(2, 1u << log2_p) && on.workgroups() == 2);
    }
    {   // 16 partials is no balanced size the option adds; 128 keeps the chunked form and the plan has no schedule bank
        const BankLaunch small = balanced_bank(2, 4, 0), big = balanced_bank(2, 7, 0);
        CHECK(!rule({&small}, 2, true).servable);
        const StreamPlan on = rule({&big}, 2, true);
        CHECK(on.servable && !on.has_general() && on.general_voices.empty() && !on.banks[0].general);
    }
    {   // a schedule bank next to other banks needs FR_STREAM_BANKS as well; voices are numbered globally
        const BankLaunch big = balanced_bank(1, 8, 0), mid = general_bank({{6, 5 | 1u << 4, 2 | 1u << 4}, {6, 5 | 1u << 4, 2 | 1u << 4}}, 1), low = balanced_bank(2, 6, 3);
        const StreamPlan alone = rule({&big, &mid, &low}, 5, true, false);
        CHECK(!alone.servable && alone.reason.find("one voice bank (this one: 3 bank launches)") != std::string::npos);
        const StreamPlan on = rule({&big, &mid, &low}, 5, true, true);
        CHECK(on.servable && on.voices == 5 && on.general_voices == (std::vector<uint32_t>{100, 100, 64, 64}));
        CHECK(on.banks.size() == 3 && !on.banks[0].general && on.banks[1].general && on.banks[2].general);
        CHECK(on.banks[1].first_voice == 1 && on.banks[2].first_voice == 3 && on.banks[1].first_wg == on.banks[0].voices << (8 - on.banks[0].chunk_log2));
        CHECK(on.workgroups() == on.banks[2].first_wg + 2);
        CHECK(!rule({&big, &mid, &low}, 5, false, true).servable);
    }
    {   // the refusals that stay: compiled and track voices, another input slot, more voices than workgroups, too many leaves
        BankLaunch jit = g;
        jit.general = false; jit.jit = true; jit.log2_p = 7;
        const StreamPlan a = rule({&jit}, 2, true);
        CHECK(!a.servable && a.reason.find("compiled or track voices") != std::string::npos && a.reason.find("general") == std::string::npos);
        BankLaunch slot = g;
        slot.input_slot = 1;
        CHECK(rule({&slot}, 2, true).reason == "block streaming feeds input slot 0; these voices read another slot");
        const BankLaunch many = general_bank(std::vector<std::vector<uint32_t>>(257, {4}));
        CHECK(rule({&many}, 257, true).reason.find("one voice per CU (256 here)") != std::string::npos);
        std::vector<uint32_t> huge(20, 11);                               // 20 items of 2048 leaves = 40960, a left chain
        for (size_t i = 1; i < huge.size(); ++i) huge[i] |= 1u << 4;
        const BankLaunch big = general_bank({huge});
        const StreamPlan b = rule({&big}, 1, true);
        CHECK(!b.servable && b.reason.find("40960 leaves") != std::string::npos && b.reason.find("32768") != std::string::npos);
        std::vector<uint32_t> most(16, 11);                               // 32768 leaves exactly: served
        for (size_t i = 1; i < most.size(); ++i) most[i] |= 1u << 4;
        const BankLaunch limit = general_bank({most});
        CHECK(rule({&limit}, 1, true).servable);
    }
    {   // a schedule that fails the validation is refused, never launched
        BankLaunch bad = g;
        bad.groups[1] = 5;                                                // voice 0 now leaves two values (its last merge pops one)
        const StreamPlan a = rule({&bad}, 2, true);
        CHECK(!a.servable && a.reason.rfind("internal: ", 0) == 0);
        const BankLaunch deep = general_bank({std::vector<uint32_t>(17, 3)});   // 17 pending operands
        const StreamPlan b = rule({&deep}, 1, true);
        CHECK(!b.servable && b.reason.rfind("internal: ", 0) == 0 && b.reason.find("deeper than 16") != std::string::npos);
        BankLaunch cut = g;
        cut.group_off.resize(4);                                          // the second voice has no entry
        CHECK(rule({&cut}, 2, true).reason.rfind("internal: ", 0) == 0);
    }
}

int main() {
    test_schedule_ok();
    test_balanced_schedules();
    test_deal();
    test_rule();
    test_model();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
