// streamrows_tests.cpp -- the row bookkeeping of streamed blocks (libfriendship_amd/csrc/streamrows.hpp) against a model that
// stores the samples the way the reference's input store does (reference.rs:47-75: vectors resized on a seek, created up to
// buff.len(), extended by the rows in order, padded with their last value).  Stand-alone: built and run on the CPU with
// -fsanitize=address,undefined by tests/test_stream_rows_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../libfriendship_amd/csrc/streamrows.hpp"

using namespace fr;

static int passed = 0, failed = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (cond) ++passed;                                                         \
        else { ++failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// The store with its samples.
struct Model {
    std::vector<std::vector<float>> inputs;
    uint64_t head = 0;
    // 0 ok, 1 too long, 2 history; a refused call changes nothing
    int fill(uint32_t n_slots, uint64_t n_times, uint64_t idx, const std::vector<std::vector<float>> &rows) {
        std::vector<std::vector<float>> in = inputs;
        if (idx != head)
            for (auto &v : in) v.assign(idx, 0.0f);
        while (in.size() < (uint64_t)n_slots * n_times) in.emplace_back(idx, 0.0f);
        for (size_t r = 0; r < rows.size() && r < in.size(); ++r) {
            if (in[r].size() != idx) return 2;
            in[r].insert(in[r].end(), rows[r].begin(), rows[r].end());
            if (in[r].size() > idx + n_times) return 1;
            const float pad = in[r].empty() ? 0.0f : in[r].back();
            in[r].resize(idx + n_times, pad);
        }
        inputs.swap(in);
        head = idx + n_times;
        return 0;
    }
    float at(uint32_t slot, uint64_t t) const { return slot < inputs.size() && t < inputs[slot].size() ? inputs[slot][t] : 0.0f; }
};

struct Csr {
    std::vector<float> data;
    std::vector<uint64_t> offs{0};
    explicit Csr(const std::vector<std::vector<float>> &rows) {
        for (const auto &r : rows) {
            data.insert(data.end(), r.begin(), r.end());
            offs.push_back(data.size());
        }
        if (data.empty()) data.push_back(0.0f);
    }
};

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// One block through both; compares status and, when accepted, what the wanted slots read at every frame of the block.
struct Pair {
    Model m;
    StreamRows s;
    uint64_t s_head = 0;
    bool s_have = false;
    explicit Pair(uint64_t vecs = 0) {
        m.inputs.assign(vecs, {});
        m.head = UINT64_MAX;           // the first call is a seek
        s.open(vecs);
    }
    int block(uint32_t n_slots, uint64_t n_times, uint64_t idx, const std::vector<std::vector<float>> &rows, const std::vector<uint32_t> &want) {
        const Csr c(rows);
        const bool seek = !s_have || idx != s_head;
        const StreamRows before = s;
        std::string why;
        const StreamRowsStatus st = s.check(n_slots, n_times, idx, seek, c.offs.data(), (uint32_t)rows.size(), &why);
        const int ms = m.fill(n_slots, n_times, idx, rows);
        CHECK((st == STREAM_ROWS_OK ? 0 : st == STREAM_ROWS_TOO_LONG ? 1 : 2) == ms);
        CHECK((st == STREAM_ROWS_OK) == why.empty());
        if (st != STREAM_ROWS_OK) {    // check() changes nothing
            CHECK(before.n_vecs == s.n_vecs && before.slots.size() == s.slots.size() && before.segs.size() == s.segs.size());
            return ms;
        }
        float out[8][STREAM_ROW_FRAMES];
        s.accept(n_slots, n_times, idx, seek, c.data.data(), c.offs.data(), (uint32_t)rows.size(), want.data(), (uint32_t)want.size(), out);
        bool ok = true;
        for (size_t j = 0; j < want.size(); ++j)
            for (uint64_t i = 0; i < STREAM_ROW_FRAMES; ++i) ok = ok && same_bits(out[j][i], i < n_times ? m.at(want[j], idx + i) : 0.0f);
        CHECK(ok);
        CHECK(s.n_vecs == m.inputs.size());
        bool lens = true;
        for (uint64_t r = 0; r < m.inputs.size() && r < 64; ++r) lens = lens && s.len_of(r) == m.inputs[r].size();
        CHECK(lens);
        s_head = idx + n_times;
        s_have = true;
        return 0;
    }
};

static std::vector<float> ramp(float a, size_t n) {
    std::vector<float> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = a + (float)i;
    return v;
}

static void test_padding() {
    Pair p;
    const std::vector<uint32_t> want{0, 1, 2};
    CHECK(p.block(2, 8, 100, {ramp(100, 8), ramp(1, 3), {}}, want) == 0);                 // short row: own last value; empty after a seek: 0
    CHECK(p.block(2, 8, 108, {ramp(108, 8), {}, {5.0f}}, want) == 0);                     // empty continuing row: the previous block's last value (3)
    CHECK(p.block(2, 4, 116, {ramp(116, 4), {}, {}}, want) == 0);                         // ... and again (3 and 5)
    CHECK(p.block(2, 4, 120, {ramp(120, 4), {-0.0f}, {NAN, INFINITY}}, want) == 0);       // -0, NaN and inf pad as they are
    CHECK(p.block(2, 4, 124, {ramp(124, 4), {}, {}}, want) == 0);
}

static void test_absent_slots() {
    Pair p;
    const std::vector<uint32_t> want{0, 1, 3};
    CHECK(p.block(4, 16, 0, {ramp(0, 16), ramp(7, 16)}, want) == 0);                      // slot 3 gets no row: +0.0
    CHECK(p.block(4, 16, 16, {ramp(16, 16)}, want) == 0);                                 // slot 1 left out: +0.0 there, and it falls behind
    CHECK(p.block(4, 16, 32, {ramp(32, 16), ramp(9, 16)}, want) == 2);                    // fed again: it no longer continues
    CHECK(p.block(4, 16, 32, {ramp(32, 16)}, want) == 0);                                 // the refused block left everything as it was
    CHECK(p.block(4, 16, 500, {ramp(500, 16), ramp(9, 16), {}, {1.0f}}, want) == 0);      // a seek: every slot starts again
    CHECK(p.block(4, 16, 20, {ramp(20, 16), {}, {}, {}}, want) == 0);                     // back: a seek too, the empty rows pad 0
}

static void test_vector_count() {
    Pair p;
    const std::vector<uint32_t> want{0, 1, 2};
    CHECK(p.block(1, 1, 40, {{40.0f}, {0.5f}, {0.25f}}, want) == 0);                      // one vector: rows 1 and 2 are dropped and read +0.0
    CHECK(p.s.n_vecs == 1);
    CHECK(p.block(1, 5, 41, {ramp(41, 5), {0.5f}, ramp(2, 6)}, want) == 1);               // now they count: row 2 is too long
    CHECK(p.s.n_vecs == 1);                                                               // ... and the refusal created no vector
    CHECK(p.block(1, 5, 41, {ramp(41, 5), {0.5f}, ramp(2, 5), {}, {}}, want) == 0);       // accepted in the next
    CHECK(p.s.n_vecs == 5);
    CHECK(p.block(1, 2, 46, {ramp(46, 2), {}, {}, {}, {}, {9.0f}, {9.0f, 9.0f, 9.0f}}, want) == 0);   // rows 5 and 6 beyond the count: dropped unchecked
    Pair q(300);                                                                          // the renderer's own count: rows are taken at once
    CHECK(q.block(1, 1, 7, {{7.0f}, {0.5f}, {0.25f}}, want) == 0);
    CHECK(q.s.n_vecs == 300);
}

static void test_refusals_change_nothing() {
    Pair p;
    const std::vector<uint32_t> want{0, 1};
    CHECK(p.block(2, 8, 0, {ramp(0, 8), {2.0f}}, want) == 0);
    CHECK(p.block(2, 8, 8, {ramp(8, 9), {}}, want) == 1);                                 // n_times + 1 values
    CHECK(p.block(2, 8, 8, {ramp(8, 8), ramp(0, 9)}, want) == 1);
    CHECK(p.block(2, 8, 8, {ramp(8, 8), {}}, want) == 0);                                 // continues as if they had not been made: pad 2
    CHECK(p.block(2, 8, 900, {ramp(900, 9)}, want) == 1);                                 // a refused seek ...
    CHECK(p.block(2, 8, 16, {ramp(16, 8), {}}, want) == 0);                               // ... is no seek: the next block still continues
    CHECK(p.block(2, 8, 24, {ramp(24, 8)}, want) == 0);
    CHECK(p.block(2, 8, 32, {ramp(32, 8), {1.0f}}, want) == 2);
    CHECK(p.block(2, 8, 32, {ramp(32, 8)}, want) == 0);
}

static void test_random_sequences() {
    std::mt19937 rng(12345);
    const float special[] = {0.0f, -0.0f, 1e-42f, INFINITY, -INFINITY, NAN, 1.5f};
    for (int seq = 0; seq < 200; ++seq) {
        Pair p(rng() % 3 == 0 ? rng() % 40 : 0);
        const uint32_t n_slots = 1 + rng() % 4;
        std::vector<uint32_t> want{0};
        for (uint32_t s = 1; s < 12; ++s)
            if (rng() % 2 && want.size() < 8) want.push_back(s);
        uint64_t idx = rng() % 1000;
        for (int b = 0; b < 30; ++b) {
            const uint64_t T = 1 + rng() % 64;
            if (rng() % 9 == 0) idx = rng() % 3000;                                       // a seek, forward or back
            std::vector<std::vector<float>> rows(rng() % 12);
            for (auto &r : rows) {
                const uint64_t len = rng() % 5 == 0 ? 0 : rng() % 17 == 0 ? T + 1 : 1 + rng() % T;
                for (uint64_t i = 0; i < len; ++i) r.push_back(rng() % 11 == 0 ? special[rng() % 7] : (float)(rng() % 2000) / 64.0f - 10.0f);
            }
            if (p.block(n_slots, T, idx, rows, want) == 0) idx += T;
        }
    }
}

int main() {
    test_padding();
    test_absent_slots();
    test_vector_count();
    test_refusals_change_nothing();
    test_random_sequences();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
