// streambanks_tests.cpp -- the chunk sizes block streaming deals to the banks of one resident launch
// (libfriendship_amd/csrc/streamplan.hpp deal_stream_chunks, FR_STREAM_BANKS) on their own: one bank against the loop the
// single-bank kernels have always had, several banks against the rule's stated properties, hand-derived answers and a model
// written the slow way.  Stand-alone: built and run on the CPU with -fsanitize=address,undefined by
// tests/test_stream_banks_host.py.
#include <cstdio>
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

static StreamBank bank(uint32_t voices, uint32_t log2_p) {
    StreamBank b;
    b.voices = voices;
    b.log2_p = log2_p;
    return b;
}

static uint64_t wgs_of(const StreamBank &b) { return (uint64_t)b.voices << (b.log2_p - b.chunk_log2); }

// The single-bank loop as fr_stream_begin and plan_stream have had it: false = refused (more voices than workgroups).
static bool todays_loop(uint32_t V, uint32_t log2_p, uint64_t max_wgs, uint32_t &c) {
    c = log2_p;
    while (c > 7 && ((uint64_t)V << (log2_p - c + 1)) <= max_wgs && log2_p - c < 8) --c;
    return ((uint64_t)V << (log2_p - c)) <= max_wgs;
}

// The rule the slow way: everything recomputed from the chunk sizes in every step, candidates collected first.
static bool model(std::vector<StreamBank> &banks, uint64_t max_wgs) {
    for (StreamBank &b : banks) b.chunk_log2 = b.log2_p;
    auto total = [&] { uint64_t t = 0; for (const StreamBank &b : banks) t += wgs_of(b); return t; };
    if (total() > max_wgs) return false;
    for (;;) {
        std::vector<size_t> ok;
        for (size_t i = 0; i < banks.size(); ++i) {
            const StreamBank &b = banks[i];
            if (b.chunk_log2 > 7 && b.log2_p - b.chunk_log2 < 8 && total() + wgs_of(b) <= max_wgs) ok.push_back(i);
        }
        if (ok.empty()) return true;
        size_t best = ok[0];
        for (size_t i : ok)
            if (banks[i].chunk_log2 > banks[best].chunk_log2) best = i;
        --banks[best].chunk_log2;
    }
}

static std::vector<uint32_t> chunks_of(std::vector<StreamBank> banks, uint64_t max_wgs, bool *ok = nullptr) {
    const bool r = deal_stream_chunks(banks, max_wgs);
    if (ok) *ok = r;
    std::vector<uint32_t> c;
    for (const StreamBank &b : banks) c.push_back(1u << (b.log2_p - b.chunk_log2));
    return c;
}

static void one_bank_is_todays_loop() {
    for (uint64_t max_wgs : {256ull, 255ull, 104ull, 64ull, 32ull, 1ull})
        for (uint32_t V = 1; V <= 256; ++V)
            for (uint32_t lp = 7; lp <= 15; ++lp) {
                uint32_t c = 0;
                const bool served = todays_loop(V, lp, max_wgs, c);
                std::vector<StreamBank> b{bank(V, lp)};
                const bool got = deal_stream_chunks(b, max_wgs);
                bool same = got == served && (!served || (b[0].chunk_log2 == c && b[0].first_wg == 0 && b[0].first_voice == 0));
                if (!same) std::printf("  V=%u log2_p=%u max_wgs=%llu: rule %d chunk_log2 %u, today's loop %d chunk_log2 %u\n", V, lp, (unsigned long long)max_wgs, got,
                                       b[0].chunk_log2, served, c);
                CHECK(same);
            }
    std::vector<StreamBank> b{bank(257, 7)};
    CHECK(!deal_stream_chunks(b, 256));
}

static void properties_of_several_banks() {
    std::mt19937 rng(0x5EED0740);
    for (int trial = 0; trial < 4000; ++trial) {
        const uint64_t max_wgs = trial % 3 == 0 ? 256 : 1 + rng() % 256;
        const size_t n = 2 + rng() % 7;
        std::vector<StreamBank> banks;
        for (size_t i = 0; i < n; ++i) banks.push_back(bank(1 + rng() % (trial % 2 ? 8 : 64), 7 + rng() % 9));
        std::vector<StreamBank> want = banks;
        const bool served = deal_stream_chunks(banks, max_wgs);
        uint64_t voices = 0;
        for (const StreamBank &b : banks) voices += b.voices;
        CHECK(served == (voices <= max_wgs));
        CHECK(model(want, max_wgs) == served);
        if (!served) continue;
        uint64_t total = 0, v = 0;
        bool fields = true, bounds = true, matches = true;
        for (size_t i = 0; i < n; ++i) {
            const StreamBank &b = banks[i];
            fields = fields && b.first_wg == total && b.first_voice == v;
            bounds = bounds && b.chunk_log2 >= 7 && b.chunk_log2 <= b.log2_p && b.log2_p - b.chunk_log2 <= 8;   // >= 128 partials, <= 256 chunks
            matches = matches && b.chunk_log2 == want[i].chunk_log2;
            total += wgs_of(b);
            v += b.voices;
        }
        CHECK(fields);
        CHECK(bounds);
        CHECK(matches);
        CHECK(total <= max_wgs);
        bool stopped = true;                       // where it stops, no bank can be halved any more
        for (const StreamBank &b : banks)
            stopped = stopped && !(b.chunk_log2 > 7 && b.log2_p - b.chunk_log2 < 8 && total + wgs_of(b) <= max_wgs);
        CHECK(stopped);
    }
}

static void pinned_answers() {
    using V = std::vector<uint32_t>;
    bool ok = false;
    // the largest chunk goes first, and a 128-partial bank is never chunked
    CHECK((chunks_of({bank(1, 10), bank(1, 7)}, 256, &ok) == V{8, 1}) && ok);
    CHECK((chunks_of({bank(2, 7), bank(2, 10)}, 256) == V{1, 8}));
    // a tie goes to the lower bank index: with room for one more workgroup only bank 0 is halved
    CHECK((chunks_of({bank(1, 10), bank(1, 10)}, 3) == V{2, 1}));
    CHECK((chunks_of({bank(1, 10), bank(1, 10)}, 4) == V{2, 2}));
    CHECK((chunks_of({bank(1, 10), bank(1, 10)}, 5) == V{2, 2}));
    CHECK((chunks_of({bank(1, 10), bank(1, 10)}, 6) == V{4, 2}));
    CHECK((chunks_of({bank(1, 10), bank(1, 10)}, 256) == V{8, 8}));
    // a bank that has no room is passed over, a smaller one behind it still halves
    CHECK((chunks_of({bank(1, 8), bank(100, 10)}, 256) == V{2, 2}));
    // a chord of 8 x 1024, 16 x 512, 32 x 256: every bank ends at 128 partials per workgroup (192 workgroups); with 104
    // workgroups, at 256
    CHECK((chunks_of({bank(8, 10), bank(16, 9), bank(32, 8)}, 256) == V{8, 4, 2}));
    CHECK((chunks_of({bank(8, 10), bank(16, 9), bank(32, 8)}, 104) == V{4, 2, 1}));
    // at most 256 chunks per voice
    CHECK((chunks_of({bank(1, 15), bank(1, 7)}, 1024) == V{256, 1}));
    // more voices than workgroups
    chunks_of({bank(200, 7), bank(100, 8)}, 256, &ok);
    CHECK(!ok);
    // an unknown device (0 CUs) has the kernel's limit, and nothing else depends on it
    CHECK(stream_max_wgs(0) == 256 && stream_max_wgs(256) == 256 && stream_max_wgs(304) == 256 && stream_max_wgs(64) == 64);
    std::mt19937 rng(7);
    for (int trial = 0; trial < 200; ++trial) {
        std::vector<StreamBank> banks;
        for (size_t i = 0, n = 2 + rng() % 7; i < n; ++i) banks.push_back(bank(1 + rng() % 16, 7 + rng() % 9));
        CHECK(chunks_of(banks, stream_max_wgs(0)) == chunks_of(banks, stream_max_wgs(256)));
    }
}

int main() {
    one_bank_is_todays_loop();
    properties_of_several_banks();
    pinned_answers();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
