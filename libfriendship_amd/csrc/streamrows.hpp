// streamrows.hpp -- the input store's rules for the rows of a streamed block (fr_stream_block_rows, FR_STREAM_INPUTS), kept as
// bookkeeping without the samples.  Plain host logic, no HIP runtime calls, all inline (as bankplan.hpp and streamplan.hpp).
//
// A stream keeps no input history: its programs read every input at the current frame only.  What fr_fill_buffer's store
// (engine.cpp store_inputs, reference.rs:47-75) would answer for the same sequence of calls still depends on the past:
//   * a supplied row must continue its slot's length exactly (else FR_ERR_INPUT_HISTORY) and may not be longer than the
//     block (FR_ERR_INPUT_TOO_LONG);
//   * a short row is padded with its own last value, an empty one with the last value the slot holds (0 after a seek);
//   * a slot that gets no row in a block reads +0.0 there, and falls behind: a later row for it no longer continues it;
//   * rows at or beyond the vector count -- n_slots * n_times of the largest call so far, the `buff.len()` quirk of
//     reference.rs:60 -- are dropped, unvalidated.
// So per slot: fed / length / last value, and the lengths of the vectors never fed as segments, as the engine's store has them.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace fr {

constexpr uint32_t STREAM_ROW_FRAMES = 64;   // (= streamplan.hpp STREAM_BLOCK)

enum StreamRowsStatus : uint8_t { STREAM_ROWS_OK, STREAM_ROWS_TOO_LONG, STREAM_ROWS_HISTORY };

struct StreamRows {
    struct Slot {
        bool fed = false;
        uint64_t len = 0;        // samples the slot's vector holds
        float last = 0.0f;       // the last of them (0: none, or the zeros a seek leaves)
    };
    struct Seg { uint64_t first, last, len; };   // vectors [first, last) were created with `len` zeros and never fed since
    uint64_t n_vecs = 0;
    std::vector<Seg> segs;
    std::vector<Slot> slots;

    // A stream opens on a renderer that has `vecs` input vectors; its first block is a seek.
    void open(uint64_t vecs) {
        n_vecs = vecs;
        segs.clear();
        slots.clear();
    }
    uint64_t implicit_len(uint64_t slot) const {
        for (const Seg &s : segs)
            if (slot >= s.first && slot < s.last) return s.len;
        return 0;
    }
    uint64_t len_of(uint64_t slot) const { return slot < slots.size() && slots[slot].fed ? slots[slot].len : implicit_len(slot); }

    // Would the store take these rows?  Changes nothing.  `seek`: the block does not continue the previous one.
    StreamRowsStatus check(uint32_t n_slots, uint64_t n_times, uint64_t idx, bool seek, const uint64_t *offs, uint32_t n_rows, std::string *why = nullptr) const {
        const uint64_t vecs_after = std::max<uint64_t>(n_vecs, (uint64_t)n_slots * n_times);
        const uint32_t rows = (uint32_t)std::min<uint64_t>(n_rows, vecs_after);
        for (uint32_t r = 0; r < rows; ++r) {
            const uint64_t cur = (seek || r >= n_vecs) ? idx : len_of(r);   // after a seek, and for vectors this block creates
            if (cur != idx) {
                if (why) *why = "input slot " + std::to_string(r) + " holds " + std::to_string(cur) + " samples, expected idx=" + std::to_string(idx);
                return STREAM_ROWS_HISTORY;
            }
            if (offs[r + 1] < offs[r] || offs[r + 1] - offs[r] > n_times) {
                if (why) *why = "input row " + std::to_string(r) + " longer than the range rendered";
                return STREAM_ROWS_TOO_LONG;
            }
        }
        return STREAM_ROWS_OK;
    }

    // Takes the rows (check() said STREAM_ROWS_OK; 1 <= n_times <= STREAM_ROW_FRAMES) and writes what the `n_want` slots in
    // `want` read in this block to out[j][0 .. STREAM_ROW_FRAMES): the row and its padding, +0.0 beyond n_times and for a slot
    // that got no row.
    void accept(uint32_t n_slots, uint64_t n_times, uint64_t idx, bool seek, const float *in_data, const uint64_t *offs, uint32_t n_rows, const uint32_t *want,
                uint32_t n_want, float (*out)[STREAM_ROW_FRAMES]) {
        if (seek) {
            slots.clear();
            segs.clear();
            if (n_vecs) segs.push_back({0, n_vecs, idx});
        }
        const uint64_t vecs = (uint64_t)n_slots * n_times;
        if (n_vecs < vecs) {
            segs.push_back({n_vecs, vecs, idx});
            n_vecs = vecs;
        }
        const uint32_t rows = (uint32_t)std::min<uint64_t>(n_rows, n_vecs);
        if (rows > slots.size()) slots.resize(rows);
        for (uint32_t j = 0; j < n_want; ++j) std::fill(out[j], out[j] + STREAM_ROW_FRAMES, 0.0f);
        for (uint32_t r = 0; r < rows; ++r) {
            Slot &s = slots[r];
            if (!s.fed) {
                s.fed = true;
                s.len = implicit_len(r);
                s.last = 0.0f;
            }
            const uint64_t rl = offs[r + 1] - offs[r];
            const float *row = rl ? in_data + offs[r] : nullptr;
            const float pad = rl ? row[rl - 1] : s.last;
            for (uint32_t j = 0; j < n_want; ++j) {
                if (want[j] != r) continue;
                for (uint64_t i = 0; i < n_times && i < STREAM_ROW_FRAMES; ++i) out[j][i] = i < rl ? row[i] : pad;
            }
            s.last = pad;
            s.len = idx + n_times;
        }
    }
};

}  // namespace fr
