// streamstore.hpp -- the input store's side of a stream that STORES what it is fed (FR_STREAM_STORE on top of FR_STREAM_PROGRAMS).
// Plain host logic, no HIP runtime calls, all inline (as streamrows.hpp and streamplan.hpp): the engine asks it and decides
// nothing itself, the host-logic simulator compiles it with the engine, tests/cpp/streamstore_tests.cpp pins its answers.
//
// With the option the resident launch (kernels.hpp bank_stream_store_kernel) appends every streamed row of every block to the
// slot's buffer in the renderer's input store, at data[head + i - base].  The store's books -- which slot is fed, how long it is,
// where its buffer starts, how much room it has -- stay on the host, and they are fr_fill_buffer's (engine.cpp store_inputs,
// make_room; reference.rs:47-75), block by block.  This header answers, and nothing else:
//   * which slots such a stream streams (stream_store_slots) and the limit;
//   * what a block does to a slot's buffer: append in place, or relaunch first (store_room: make_room's three branches;
//     stream_store_block); how a bounded history's floor rises (store_floor);
//   * how streamrows.hpp's books are opened FROM the store's state when a stream's first block continues the renderer's head
//     (stream_rows_from_store), and how the store's books follow an accepted block (stream_store_feed, stream_store_commit);
//   * when the option is inert (stream_store_inert).
// A RELAUNCH is not a seek: the launch is stopped clean, the store does what make_room does, the launch restarts at head = idx
// with the new pointers; the rings and the stream's own history are untouched and valid.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "streamplan.hpp"
#include "streamrows.hpp"

namespace fr {

// One input slot's books in the store (engine.cpp InSlot is this and the buffer).
struct StoreSlot {
    bool fed = false;        // ever received a row (otherwise implicit zeros)
    uint64_t base = 0;       // zero prefix (seek / late creation), data[i] is time base+i
    uint64_t len = 0;        // logical length (== base + stored samples)
    uint64_t cap = 0;        // capacity in floats
};

// Frames of input history a renderer keeps per slot (0: everything since the last seek): fr_config.history_frames, and at least
// what the plan's delays can reach.
inline uint64_t store_keep_frames(uint64_t history_frames, bool plan_valid, uint64_t input_lookback) {
    if (!history_frames) return 0;
    return std::max<uint64_t>(history_frames, plan_valid ? input_lookback : 0);
}

// Bounded history: samples before the floor read 0.0.  A call (a block) at idx raises it to idx - keep; it never falls.
inline uint64_t store_floor(uint64_t floor, uint64_t keep, uint64_t idx) { return keep && idx > keep ? std::max(floor, idx - keep) : floor; }

// Room for n_times more frames behind `stored` frames in a buffer of `cap`: they fit; or (bounded history) the newest `kept`
// frames SLIDE to the front of the same buffer -- source and destination do not overlap --; or they MOVE into a new buffer of
// `cap` floats (bounded: 2 * (keep + call), at least 2^16; unbounded: twice the old one, at least 2^20).  `drop`: the frames
// that leave the front (base += drop).
struct StoreRoom {
    enum Kind : uint8_t { fits, slide, move } kind = fits;
    uint64_t drop = 0, kept = 0, cap = 0;
};
inline StoreRoom store_room(uint64_t stored, uint64_t cap, uint64_t keep, uint64_t n_times) {
    StoreRoom r;
    r.cap = cap;
    r.kept = stored;
    if (stored + n_times <= cap) return r;
    if (keep && stored > keep) {
        const uint64_t drop = stored - keep;
        if (drop >= keep && keep + n_times <= cap) {
            r.kind = StoreRoom::slide;
            r.drop = drop;
            r.kept = keep;
            return r;
        }
    }
    r.kind = StoreRoom::move;
    r.kept = keep ? std::min(stored, keep) : stored;
    r.drop = stored - r.kept;
    r.cap = keep ? std::max<uint64_t>(2 * (keep + n_times), 1u << 16) : std::max<uint64_t>(stored + n_times, std::max<uint64_t>(cap * 2, 1u << 20));
    return r;
}

// Why the option does nothing for this renderer ("": it acts).  The stream then behaves as without it.
inline std::string stream_store_inert(bool delay_observed, bool tracks_declared) {
    if (delay_observed) return "FR_DELAY_OBSERVED=1: streamed rows would escape the observed bounds";
    if (tracks_declared) return "declared track slots";
    return "";
}

// The rows of a block that the store takes: rows at or beyond the vector count after the block are dropped (reference.rs:59-68).
inline uint32_t store_rows_taken(uint64_t n_vecs, uint32_t n_slots, uint64_t n_times, uint32_t n_rows) {
    return (uint32_t)std::min<uint64_t>(n_rows, std::max<uint64_t>(n_vecs, (uint64_t)n_slots * n_times));
}

// The slots a store-mode stream streams: the plan's (StreamPlan::input_slots), every slot the store has fed, and the `rows_fed`
// slots [0, rows_fed) the block at hand feeds; slot 0 first, the others ascending.  False with more than STREAM_MAX_INPUTS.
template <class Slots>
inline bool stream_store_slots(const std::vector<uint32_t> &plan_slots, const Slots &store, uint32_t rows_fed, std::vector<uint32_t> &out, std::string *why = nullptr) {
    out.assign(plan_slots.begin(), plan_slots.end());
    for (uint32_t r = 0; r < store.size(); ++r)
        if (store[r].fed) out.push_back(r);
    for (uint32_t r = 0; r < rows_fed; ++r) out.push_back(r);
    out.push_back(0);
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    if (out.size() > STREAM_MAX_INPUTS) {
        if (why)
            *why = "a stream that stores its rows streams every input slot the plan reads, the store holds or the block feeds: " + std::to_string(out.size()) +
                   " slots here; block streaming feeds at most " + std::to_string(STREAM_MAX_INPUTS);
        return false;
    }
    return true;
}

// A launched slot: the slot, and whether the launch has its buffer (StreamStoreArgs::Row::data != null).  A launch gives a
// buffer to exactly the slots its first block feeds: a slot without a row in a block lags from then on and "can only be fed
// again after a seek", which is a launch.
struct StoreStreamed {
    uint32_t slot = 0;
    bool has_data = false;
};

// What the block [idx, idx + n_times) with rows for the slots [0, rows_fed) does to a running launch: append in place, or
// relaunch first (`why` says for what).  The rows were checked (streamrows.hpp): a fed slot's len is idx.
template <class Slots>
inline bool stream_store_block_relaunches(const std::vector<StoreStreamed> &streamed, const Slots &store, uint32_t rows_fed, uint64_t keep, uint64_t idx, uint64_t n_times,
                                          std::string *why = nullptr) {
    auto say = [&](const std::string &w) { if (why) *why = w; return true; };
    for (uint32_t r = 0; r < rows_fed; ++r) {
        auto it = std::find_if(streamed.begin(), streamed.end(), [&](const StoreStreamed &s) { return s.slot == r; });
        if (it == streamed.end()) return say("the set of streamed slots grows by slot " + std::to_string(r));
        if (!it->has_data || r >= store.size() || !store[r].fed) return say("slot " + std::to_string(r) + " is fed and the launch has no buffer of it");
    }
    for (const StoreStreamed &s : streamed) {
        if (!s.has_data) continue;
        const StoreSlot &b = store[s.slot];
        if (s.slot < rows_fed) {
            const StoreRoom room = store_room(b.len - b.base, b.cap, keep, n_times);
            if (room.kind == StoreRoom::slide) return say("slot " + std::to_string(s.slot) + "'s history slides");
            if (room.kind == StoreRoom::move) return say("slot " + std::to_string(s.slot) + "'s buffer grows");
        } else if (idx + n_times - b.base > b.cap) {   // (its rows are stored beyond its length and never read: the launch lets go of the buffer)
            return say("slot " + std::to_string(s.slot) + " lags and its buffer is full");
        }
    }
    return false;
}

// streamrows.hpp's books opened from the store's state (a stream whose first block continues the renderer's head): per slot
// fed, len and the last stored value (`last[r]`: data[len - 1 - base] of a fed slot that holds samples, else 0), the segments
// and the vector count.
template <class Slots, class Segs>
inline void stream_rows_from_store(StreamRows &rows, uint64_t n_vecs, const Segs &segs, const Slots &store, const std::vector<float> &last) {
    rows.n_vecs = n_vecs;
    rows.segs.clear();
    for (const auto &s : segs) rows.segs.push_back({s.first, s.last, s.len});
    rows.slots.assign(store.size(), StreamRows::Slot{});
    for (size_t r = 0; r < store.size(); ++r) {
        if (!store[r].fed) continue;
        rows.slots[r].fed = true;
        rows.slots[r].len = store[r].len;
        rows.slots[r].last = r < last.size() && store[r].len > store[r].base ? last[r] : 0.0f;
    }
}

// The store's seek (store_inputs): every slot empty at idx, the vectors one segment.
template <class Slots, class Segs>
inline void stream_store_seek(Slots &store, Segs &segs, uint64_t n_vecs, uint64_t idx) {
    for (auto &s : store) { s.base = idx; s.len = idx; }
    segs.clear();
    if (n_vecs) segs.push_back({0, n_vecs, idx});
}

// The slots [0, rows_fed) become fed where they were not (store_inputs: base = len = the vector's implicit length, which the
// check has found to be idx).  Before the launch gets their buffers; a block that is then refused leaves them answering what
// they answered unfed.
template <class Slots>
inline void stream_store_feed(Slots &store, uint32_t rows_fed, uint64_t idx) {
    if (rows_fed > store.size()) store.resize(rows_fed);
    for (uint32_t r = 0; r < rows_fed; ++r)
        if (!store[r].fed) { store[r].fed = true; store[r].base = idx; store[r].len = idx; }
}

// An answered block: the fed slots are as long as the block's end, the segments and the vector count are the rows' books'.
template <class Slots, class Segs>
inline void stream_store_commit(Slots &store, Segs &segs, uint64_t &n_vecs, const StreamRows &rows, uint32_t rows_fed, uint64_t idx, uint64_t n_times) {
    for (uint32_t r = 0; r < rows_fed && r < store.size(); ++r) store[r].len = idx + n_times;
    segs.clear();
    for (const StreamRows::Seg &s : rows.segs) segs.push_back({s.first, s.last, s.len});
    n_vecs = rows.n_vecs;
}

}  // namespace fr
