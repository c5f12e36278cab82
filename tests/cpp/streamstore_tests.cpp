// streamstore_tests.cpp -- the input store's side of a stream that stores what it is fed (libfriendship_amd/csrc/streamstore.hpp):
// the slots such a stream streams and their limit; append or relaunch at every boundary of make_room's three branches, for a
// bounded and an unbounded history; the floor; streamrows.hpp's books opened FROM a store state and kept up block by block, against
// a model that stores the samples the way the reference's input store does (reference.rs:47-75), over 200 random sequences of
// calls, blocks, seeks and re-openings; the inert reasons.  Stand-alone: built and run on the CPU with
// -fsanitize=address,undefined by tests/test_stream_store_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../libfriendship_amd/csrc/streamstore.hpp"

using namespace fr;

static int passed = 0, failed = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (cond) ++passed;                                                         \
        else { ++failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

struct Seg { uint64_t first, last, len; };

static std::vector<StoreSlot> fed_slots(std::initializer_list<uint32_t> fed, size_t n) {
    std::vector<StoreSlot> s(n);
    for (uint32_t r : fed) s[r].fed = true;
    return s;
}

static void test_slot_set() {
    std::vector<uint32_t> out;
    std::string why;
    CHECK(stream_store_slots({0}, fed_slots({}, 0), 0, out) && out == std::vector<uint32_t>({0}));
    CHECK(stream_store_slots({0, 5}, fed_slots({1, 3}, 4), 0, out) && out == std::vector<uint32_t>({0, 1, 3, 5}));
    CHECK(stream_store_slots({0, 5}, fed_slots({1, 3}, 4), 3, out) && out == std::vector<uint32_t>({0, 1, 2, 3, 5}));   // the block feeds 0, 1, 2
    CHECK(stream_store_slots({0}, fed_slots({2}, 3), 1, out) && out == std::vector<uint32_t>({0, 2}));                   // slot 0 first also when it is not fed
    CHECK(stream_store_slots({0, 9, 2}, fed_slots({}, 0), 0, out) && out == std::vector<uint32_t>({0, 2, 9}));           // ascending
    CHECK(stream_store_slots({0}, fed_slots({}, 0), 8, out) && out.size() == 8);                                         // exactly the limit
    CHECK(!stream_store_slots({0}, fed_slots({}, 0), 9, out, &why) && why.find("9 slots") != std::string::npos && why.find("at most 8") != std::string::npos);
    CHECK(!stream_store_slots({0, 20}, fed_slots({1, 2, 3, 4, 5, 6, 7}, 8), 0, out, &why) && why.find("9 slots") != std::string::npos);
    CHECK(STREAM_MAX_INPUTS == 8 && STREAM_MAX_INPUTS == BANK_STREAM_ROWS);
}

// make_room as the engine has always had it, written out again: what store_room must answer.
static StoreRoom make_room_model(uint64_t stored, uint64_t cap, uint64_t keep, uint64_t n) {
    StoreRoom r;
    r.cap = cap; r.kept = stored;
    if (stored + n <= cap) return r;
    if (keep && stored > keep && stored - keep >= keep && keep + n <= cap) { r.kind = StoreRoom::slide; r.drop = stored - keep; r.kept = keep; return r; }
    r.kind = StoreRoom::move;
    r.kept = keep ? (stored < keep ? stored : keep) : stored;
    r.drop = stored - r.kept;
    const uint64_t grown = cap * 2 > (1u << 20) ? cap * 2 : (1u << 20);
    r.cap = keep ? (2 * (keep + n) > (1u << 16) ? 2 * (keep + n) : (1u << 16)) : (stored + n > grown ? stored + n : grown);
    return r;
}

static void test_room() {
    // unbounded: fits up to the capacity, then doubles (at least 2^20, at least what is needed)
    CHECK(store_room(0, 0, 0, 64).kind == StoreRoom::move && store_room(0, 0, 0, 64).cap == (1u << 20) && store_room(0, 0, 0, 64).kept == 0);
    const uint64_t M = 1u << 20;
    CHECK(store_room(M - 64, M, 0, 64).kind == StoreRoom::fits);
    CHECK(store_room(M - 63, M, 0, 64).kind == StoreRoom::move && store_room(M - 63, M, 0, 64).cap == 2 * M && store_room(M - 63, M, 0, 64).kept == M - 63 &&
          store_room(M - 63, M, 0, 64).drop == 0);
    CHECK(store_room(M, M, 0, 3 * M).cap == 4 * M);
    // bounded, keep = 256: the buffer is max(2 * (keep + call), 2^16); full: the newest 256 slide to the front
    const uint64_t B = 1u << 16;
    CHECK(store_room(0, 0, 256, 64).kind == StoreRoom::move && store_room(0, 0, 256, 64).cap == B);
    CHECK(store_room(B - 64, B, 256, 64).kind == StoreRoom::fits);
    const StoreRoom s = store_room(B - 63, B, 256, 64);
    CHECK(s.kind == StoreRoom::slide && s.drop == B - 63 - 256 && s.kept == 256 && s.cap == B);
    // ... a slide needs source and destination apart (drop >= keep) and room for keep + call; else a new buffer
    CHECK(store_room(300, 320, 256, 64).kind == StoreRoom::move && store_room(300, 320, 256, 64).kept == 256 && store_room(300, 320, 256, 64).drop == 44);
    CHECK(store_room(600, 610, 256, 64).kind == StoreRoom::slide);
    CHECK(store_room(600, 310, 256, 64).kind == StoreRoom::move);            // keep + call > cap
    CHECK(store_room(100, 120, 256, 64).kind == StoreRoom::move && store_room(100, 120, 256, 64).kept == 100 && store_room(100, 120, 256, 64).drop == 0);
    CHECK(store_room(10, 20, 40000, 64).cap == 2 * (40000 + 64));
    std::mt19937_64 rng(7);
    for (int i = 0; i < 20000; ++i) {
        const uint64_t keep = rng() % 3 == 0 ? 0 : 1 + rng() % 700, cap = rng() % 3000, stored = cap ? rng() % (cap + 1) : 0, n = 1 + rng() % 64;
        const StoreRoom a = store_room(stored, cap, keep, n), b = make_room_model(stored, cap, keep, n);
        CHECK(a.kind == b.kind && a.drop == b.drop && a.kept == b.kept && a.cap == b.cap);
        CHECK(a.kept + n <= a.cap && a.drop + a.kept == stored);             // what stays and the call fit; nothing is lost but the dropped front
        if (a.kind == StoreRoom::slide) CHECK(a.drop >= a.kept);             // source and destination do not overlap
    }
}

static void test_floor_and_keep() {
    CHECK(store_floor(0, 0, 100000) == 0);                                   // unbounded: no floor
    CHECK(store_floor(0, 256, 256) == 0 && store_floor(0, 256, 257) == 1 && store_floor(0, 256, 1000) == 744);
    CHECK(store_floor(900, 256, 1000) == 900);                               // it never falls
    uint64_t by_block = 0, by_call = 0;
    for (uint64_t idx = 0; idx < 5000; idx += 64) by_block = store_floor(by_block, 256, idx);
    by_call = store_floor(by_call, 256, 4992);
    CHECK(by_block == by_call && by_block == 4992 - 256);                    // per block as store_inputs raises it per call
    CHECK(store_keep_frames(0, true, 500) == 0 && store_keep_frames(256, true, 100) == 256 && store_keep_frames(256, true, 500) == 500 &&
          store_keep_frames(256, false, 500) == 256);
}

static void test_block_decision() {
    const uint64_t B = 1u << 16;
    std::vector<StoreSlot> store(3);
    store[0] = {true, 0, 1000, B};
    store[1] = {true, 0, 1000, B};
    store[2] = {true, 0, 400, B};                                            // lags
    std::vector<StoreStreamed> streamed{{0, true}, {1, true}, {2, false}};
    std::string why;
    CHECK(!stream_store_block_relaunches(streamed, store, 2, 0, 1000, 64));
    CHECK(stream_store_block_relaunches(streamed, store, 3, 0, 1000, 64, &why) && why.find("no buffer") != std::string::npos);   // a row for a slot the launch has no buffer of
    CHECK(stream_store_block_relaunches(std::vector<StoreStreamed>{{0, true}}, store, 2, 0, 1000, 64, &why) && why.find("grows by slot 1") != std::string::npos);
    // the room, at the boundary of each branch
    store[0].len = store[1].len = B - 64;
    CHECK(!stream_store_block_relaunches(streamed, store, 2, 256, B - 64, 64));
    CHECK(!stream_store_block_relaunches(streamed, store, 2, 0, B - 64, 64));
    store[0].len = store[1].len = B - 63;
    CHECK(stream_store_block_relaunches(streamed, store, 2, 256, B - 63, 64, &why) && why.find("slides") != std::string::npos);
    CHECK(stream_store_block_relaunches(streamed, store, 2, 0, B - 63, 64, &why) && why.find("grows") != std::string::npos);
    CHECK(!stream_store_block_relaunches(streamed, store, 2, 0, B - 63, 63));
    // a slot with a buffer that gets no row any more: its rows still land in the buffer, so it needs the room too
    store[0].len = B - 32; store[1].len = 5000;
    CHECK(!stream_store_block_relaunches(streamed, store, 1, 0, B - 32, 32));
    CHECK(stream_store_block_relaunches(streamed, store, 1, 0, B - 32, 33, &why));
    store[0].len = 6000; store[0].cap = 2 * B;
    CHECK(!stream_store_block_relaunches(streamed, store, 1, 0, B - 64, 64));
    CHECK(stream_store_block_relaunches(streamed, store, 1, 0, B - 63, 64, &why) && why.find("lags") != std::string::npos);
    // a base: positions count from it
    store[0] = {true, 5000, 5000 + B - 64, B};
    CHECK(!stream_store_block_relaunches(std::vector<StoreStreamed>{{0, true}}, store, 1, 0, 5000 + B - 64, 64));
    CHECK(stream_store_block_relaunches(std::vector<StoreStreamed>{{0, true}}, store, 1, 0, 5000 + B - 64, 64 + 1));
}

static void test_inert() {
    CHECK(stream_store_inert(false, false).empty());
    CHECK(stream_store_inert(true, false) == "FR_DELAY_OBSERVED=1: streamed rows would escape the observed bounds");
    CHECK(stream_store_inert(false, true) == "declared track slots");
    CHECK(store_rows_taken(0, 2, 64, 5) == 5 && store_rows_taken(0, 1, 1, 5) == 1 && store_rows_taken(300, 1, 1, 5) == 5);
}

// The store with its samples (reference.rs:47-75).
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
    float at(uint64_t slot, uint64_t t) const { return slot < inputs.size() && t < inputs[slot].size() ? inputs[slot][t] : 0.0f; }
};

static bool same(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

// The engine's side: the store's books (no samples), driven through the header alone, with streamrows.hpp's books re-opened from
// them at random moments -- as a stream is opened on a renderer that fr_fill_buffer and earlier streams have fed.
struct Engine {
    std::vector<StoreSlot> store;
    std::vector<Seg> segs;
    uint64_t n_vecs = 0, head = 0;
    StreamRows rows;
    bool open = false;
    void reopen(const Model &m) {
        std::vector<float> last(store.size(), 0.0f);
        for (size_t r = 0; r < store.size(); ++r)
            if (store[r].fed && store[r].len > store[r].base) last[r] = m.at(r, store[r].len - 1);      // the one D2H per fed slot
        rows = StreamRows{};
        stream_rows_from_store(rows, n_vecs, segs, store, last);
        open = true;
    }
    int block(const Model &before, uint32_t n_slots, uint64_t n_times, uint64_t idx, const std::vector<std::vector<float>> &in, const std::vector<uint32_t> &want,
              float (*out)[STREAM_ROW_FRAMES]) {
        const bool seek = idx != head;
        if (!seek && !open) reopen(before);
        std::vector<float> data;
        std::vector<uint64_t> offs{0};
        for (const auto &r : in) { data.insert(data.end(), r.begin(), r.end()); offs.push_back(data.size()); }
        if (!open) { rows = StreamRows{}; rows.open(n_vecs); open = true; }
        const StreamRowsStatus st = rows.check(n_slots, n_times, idx, seek, offs.data(), (uint32_t)in.size());
        if (st != STREAM_ROWS_OK) return st == STREAM_ROWS_TOO_LONG ? 1 : 2;
        const uint32_t fed = store_rows_taken(rows.n_vecs, n_slots, n_times, (uint32_t)in.size());
        if (seek) stream_store_seek(store, segs, n_vecs, idx);
        stream_store_feed(store, fed, idx);
        rows.accept(n_slots, n_times, idx, seek, data.data(), offs.data(), (uint32_t)in.size(), want.data(), (uint32_t)want.size(), out);
        stream_store_commit(store, segs, n_vecs, rows, fed, idx, n_times);
        head = idx + n_times;
        return 0;
    }
};

static void test_books_follow_the_store() {
    const float special[7] = {0.0f, -0.0f, INFINITY, -INFINITY, NAN, 1e-42f, 4294967808.0f};
    for (uint64_t seed = 1; seed <= 200; ++seed) {
        std::mt19937_64 rng(seed);
        Model m;
        Engine e;
        uint64_t idx = 0;
        const uint32_t n_slots = 1 + rng() % 3;
        const std::vector<uint32_t> want{0, 1, 2, 3, 5};
        for (int call = 0; call < 60; ++call) {
            const uint64_t T = 1 + rng() % 64;
            if (rng() % 11 == 0) idx = rng() % 3000;                                         // a seek, forward or back
            if (rng() % 6 == 0) e.open = false;                                              // the stream is closed; the next block opens one from the store
            std::vector<std::vector<float>> in(rng() % 7);
            for (auto &r : in) {
                const uint64_t len = rng() % 5 == 0 ? 0 : rng() % 17 == 0 ? T + 1 : 1 + rng() % T;
                for (uint64_t i = 0; i < len; ++i) r.push_back(rng() % 11 == 0 ? special[rng() % 7] : (float)(rng() % 2000) / 64.0f - 10.0f);
            }
            float out[5][STREAM_ROW_FRAMES];
            const Model before = m;
            const int a = m.fill(n_slots, T, idx, in);
            const int b = e.block(before, n_slots, T, idx, in, want, out);
            CHECK(a == b);
            if (a != 0 || b != 0) continue;
            for (size_t j = 0; j < want.size(); ++j)
                for (uint64_t i = 0; i < STREAM_ROW_FRAMES; ++i) {
                    const float exp = i < T ? m.at(want[j], idx + i) : 0.0f;
                    if (!same(out[j][i], exp)) { CHECK(same(out[j][i], exp)); break; }
                }
            // the books: every vector as long as the model's, through the rows' books and through the store's
            CHECK(e.n_vecs == m.inputs.size() && e.rows.n_vecs == e.n_vecs);
            bool ok = true;
            for (uint64_t r = 0; r < m.inputs.size() && r < 16; ++r) {
                ok = ok && e.rows.len_of(r) == m.inputs[r].size();
                uint64_t implicit = 0;
                for (const Seg &s : e.segs) if (r >= s.first && r < s.last) implicit = s.len;
                const uint64_t len = r < e.store.size() && e.store[r].fed ? e.store[r].len : implicit;
                ok = ok && len == m.inputs[r].size();
                if (r < e.store.size() && e.store[r].fed)                                        // before its base a fed slot is zeros
                    for (uint64_t t = 0; t < e.store[r].base && t < m.inputs[r].size(); t += 97) ok = ok && same(m.inputs[r][t], 0.0f);
            }
            CHECK(ok);
            idx += T;
        }
        CHECK(passed > 0);
    }
}

int main() {
    test_slot_set();
    test_room();
    test_floor_and_keep();
    test_block_decision();
    test_inert();
    test_books_follow_the_store();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
