// leafprog.hpp -- the leaf of a shape-matched voice as a short register program (FR_STREAM_LEAVES, streamplan.hpp).
//
// fr_fill_buffer renders a compiled voice with a hipRTC-generated kernel (jit.hpp, leafjit.cpp).  A resident streaming launch
// cannot be generated per patch -- its body is protocol, written once -- so it INTERPRETS the leaf: the same four inputs that
// generate_leaf_source takes (the shape, which constant columns vary, the literals' bits, the aliased columns) become one
// instruction per arithmetic op of the shape, over registers the host allocates.  Nothing is folded: one separately rounded
// operation per primitive node, so the bits are the graph's by construction.  Plain host logic, no HIP: the rule
// (streamplan.hpp), the engine's upload and the tests share it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "leafshape.hpp"

namespace fr {

constexpr uint32_t LEAF_PROG_MAX_INSTRS = 32;   // (= kernels.hpp BANK_STREAM_LEAF_INSTRS)
constexpr uint32_t LEAF_PROG_MAX_REGS = 8;      // (= kernels.hpp BANK_STREAM_LEAF_REGS: 8 registers x 64 lanes x 16 waves = 32 KiB of LDS)
constexpr uint32_t LEAF_PROG_MAX_TRACKS = 4;    // (= kernels.hpp BANK_STREAM_LEAF_TRACKS: the distinct track rows a leaf reads, FR_STREAM_TRACKS)

// Where an operand comes from.
enum LeafOperand : uint32_t {
    LEAF_REG = 0,     // a register: the result of an earlier instruction
    LEAF_PARAM = 1,   // column `v` of the partial's row of the bank's parameter table [voice][P][k]: uniform per partial
    LEAF_LIT = 2,     // the literal with the bits `v`
    LEAF_IN = 3,      // input `v` at the lane's frame: an index into LeafProgram::input_slots (the engine's upload: the streamed row)
    // FR_STREAM_TRACKS (compile_leaf_program's allow_tracks) -- a TRACK row of the block's dense matrix at the lane's frame:
    LEAF_TRK = 4,     // ... the row whose slot number's bits stand in parameter column `v` of the partial's row (a per-partial track)
    LEAF_TRK_LIT = 5, // ... the row of slot `v`, the same for every partial
    // (the engine's upload rewrites both to LEAF_TRK with `v` = the operand's place in LeafProgram::track_cols: the column the
    //  rendering wave parked that row in)
};
// The arithmetic ops are FlatOp's numbers (graph.hpp; kernels.hip prim_binop takes them as they are).
constexpr uint32_t LEAF_OP_SUM2 = 3, LEAF_OP_MUL = 4, LEAF_OP_DIV = 5, LEAF_OP_MOD = 6, LEAF_OP_MIN = 7;

struct LeafInstr {    // 16 bytes: one uint4 of the device's copy
    uint8_t op, dst, ka, kb;   // dst = a op b; ka, kb: LeafOperand
    uint32_t a, b;
    uint32_t pad;
};
static_assert(sizeof(LeafInstr) == 16, "a leaf instruction is one uint4");

struct LeafProgram {
    std::vector<LeafInstr> ins;
    uint32_t regs = 0;                    // registers the program uses (<= LEAF_PROG_MAX_REGS)
    uint32_t k = 1;                       // floats per partial in the parameter table (generate_leaf_source's k)
    uint32_t result_kind = LEAF_REG;      // the leaf's value: the last instruction's register -- or, for a leaf that is a bare
    uint32_t result = 0;                  // constant or input, that operand
    std::vector<uint32_t> input_slots;    // the shape's external input slots: LEAF_IN operands index it
    uint32_t inputs_read = 0;             // ... of which the program reads this many distinct ones
    struct TrackCol {                     // a distinct track operand: LEAF_TRK's parameter column, or LEAF_TRK_LIT's slot
        uint32_t v;
        bool literal;
        bool operator==(const TrackCol &o) const { return v == o.v && literal == o.literal; }
    };
    std::vector<TrackCol> track_cols;     // ... in program order (<= LEAF_PROG_MAX_TRACKS; empty without allow_tracks)
    uint32_t track_index(uint32_t kind, uint32_t v) const {   // the place of a track operand in track_cols (track_cols.size(): none)
        return (uint32_t)(std::find(track_cols.begin(), track_cols.end(), TrackCol{v, kind == LEAF_TRK_LIT}) - track_cols.begin());
    }
};

// The program of a bank's leaf.  `varying`, `literal_bits`, `alias`: per constant column, as for generate_leaf_source -- a column
// that varies is parameter pidx (aliased columns share one), any other is its literal.  False, with the sentence in `why`: a track
// leaf, a malformed shape, or more instructions / registers than the interpreter has.  `allow_tracks` (FR_STREAM_TRACKS): a
// LEAF_TRACK op is an operand of kind LEAF_TRK (its column varies: aliased columns share one) or LEAF_TRK_LIT (its column is a
// literal: one slot for all partials), listed once in track_cols; more than LEAF_PROG_MAX_TRACKS distinct ones are refused.
inline bool compile_leaf_program(const LeafShape &shape, const std::vector<bool> &varying, const std::vector<uint32_t> &literal_bits, const std::vector<uint32_t> &alias,
                                 LeafProgram &out, std::string *why = nullptr, bool allow_tracks = false) {
    auto bad = [&](const std::string &w) { if (why) *why = w; return false; };
    out = LeafProgram{};
    const size_t n = shape.ops.size();
    if (n == 0) return bad("internal: a leaf without ops");
    if (varying.size() < shape.n_consts || literal_bits.size() < shape.n_consts || alias.size() < shape.n_consts) return bad("internal: a leaf shape without its columns");
    // the parameter of every varying column, in generate_leaf_source's numbering
    uint32_t k = 0;
    std::vector<int64_t> pidx(shape.n_consts, -1);
    for (uint32_t c = 0; c < shape.n_consts; ++c)
        if (varying[c]) {
            if (alias[c] > c || (alias[c] != c && pidx[alias[c]] < 0)) return bad("internal: a leaf column aliased to a later or a literal column");
            pidx[c] = alias[c] == c ? (int64_t)k++ : pidx[alias[c]];
        }
    uint32_t n_arith = 0;
    for (size_t i = 0; i < n; ++i) {
        const LeafShape::Op &o = shape.ops[i];
        if (o.op == LEAF_TRACK && !allow_tracks) return bad("a leaf reads a per-leaf track row (a track voice); block streaming interprets leaves over constants and streamed input rows only");
        if (o.op == 0u || o.op == LEAF_TRACK) {
            if (o.a >= shape.n_consts) return bad("internal: a leaf constant without a column");
        } else if (o.op == 1u) {
            if (o.a >= shape.input_slots.size()) return bad("internal: a leaf input without a slot");
        } else if (o.op >= LEAF_OP_SUM2 && o.op <= LEAF_OP_MIN) {
            if (o.a >= i || o.b >= i) return bad("internal: a leaf shape that is not in post-order");
            ++n_arith;
        } else {
            return bad("internal: a leaf op the interpreter does not know");
        }
    }
    if (n_arith > LEAF_PROG_MAX_INSTRS)
        return bad("a leaf of " + std::to_string(n_arith) + " arithmetic ops; block streaming interprets leaves of at most " + std::to_string(LEAF_PROG_MAX_INSTRS));
    // registers over the post-order list: an op's register is free again after its last reader (the result: never), and an
    // instruction may write the register of an operand it reads last -- the interpreter reads both operands before it writes
    std::vector<size_t> last_use(n, 0);
    for (size_t i = 0; i < n; ++i)
        if (shape.ops[i].op >= LEAF_OP_SUM2 && shape.ops[i].op != LEAF_TRACK) { last_use[shape.ops[i].a] = i; last_use[shape.ops[i].b] = i; }
    last_use[n - 1] = n;
    std::vector<int64_t> reg_of(n, -1);
    std::vector<bool> busy;
    std::vector<bool> in_read(shape.input_slots.size(), false);
    auto operand = [&](uint32_t i, uint8_t &kind, uint32_t &v) {
        const LeafShape::Op &o = shape.ops[i];
        if (o.op == 0u) {
            kind = varying[o.a] ? LEAF_PARAM : LEAF_LIT;
            v = varying[o.a] ? (uint32_t)pidx[o.a] : literal_bits[o.a];
        } else if (o.op == 1u) {
            kind = LEAF_IN;
            v = o.a;
            in_read[o.a] = true;
        } else if (o.op == LEAF_TRACK) {
            kind = varying[o.a] ? LEAF_TRK : LEAF_TRK_LIT;
            v = varying[o.a] ? (uint32_t)pidx[o.a] : literal_bits[o.a];
            if (out.track_index(kind, v) == out.track_cols.size()) out.track_cols.push_back({v, kind == LEAF_TRK_LIT});
        } else {
            kind = LEAF_REG;
            v = (uint32_t)reg_of[i];
        }
    };
    uint32_t peak = 0;
    for (size_t i = 0; i < n; ++i) {
        const LeafShape::Op &o = shape.ops[i];
        if (o.op < LEAF_OP_SUM2 || o.op == LEAF_TRACK) continue;
        LeafInstr in{};
        in.op = (uint8_t)o.op;
        operand(o.a, in.ka, in.a);
        operand(o.b, in.kb, in.b);
        for (uint32_t src : {o.a, o.b})
            if (reg_of[src] >= 0 && last_use[src] == i) busy[(size_t)reg_of[src]] = false;
        size_t r = 0;
        while (r < busy.size() && busy[r]) ++r;
        if (r == busy.size()) busy.push_back(false);
        busy[r] = true;
        reg_of[i] = (int64_t)r;
        in.dst = (uint8_t)r;
        peak = std::max<uint32_t>(peak, (uint32_t)busy.size());
        out.ins.push_back(in);
    }
    if (peak > LEAF_PROG_MAX_REGS)
        return bad("a leaf that needs " + std::to_string(peak) + " registers; block streaming interprets leaves with at most " + std::to_string(LEAF_PROG_MAX_REGS));
    uint8_t rk = LEAF_REG;
    operand((uint32_t)(n - 1), rk, out.result);
    out.result_kind = rk;
    if (out.track_cols.size() > LEAF_PROG_MAX_TRACKS)
        return bad("a leaf that reads " + std::to_string(out.track_cols.size()) + " distinct track rows; block streaming interprets leaves with at most " + std::to_string(LEAF_PROG_MAX_TRACKS));
    out.regs = peak;
    out.k = k ? k : 1;
    out.input_slots = shape.input_slots;
    for (bool r : in_read) out.inputs_read += r ? 1u : 0u;
    return true;
}

}  // namespace fr
