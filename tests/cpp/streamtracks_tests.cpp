// streamtracks_tests.cpp -- FR_STREAM_TRACKS on the host (libfriendship_amd/csrc/leafprog.hpp, streamplan.hpp, kernels.hpp):
//   * compile_leaf_program on the leaf BankMatcher makes of synth.track_tree's partial (the 11-node oscillator whose w and amp are
//     track rows): within 32 instructions and 8 registers, 2 track columns (w stands twice in the tree form: one aliased column),
//     refused with today's sentence when allow_tracks is false; hand-built shapes with 4 and 5 track operands, an aliased track
//     column, a literal slot, a leaf that is a bare track;
//   * a plain-loop model of kernels.hip stream_render_leaves<true> -- a wave loads the rows of partial j + 1 while it interprets
//     partial j, parks them in half j & 1 of its double buffer, the operand switch reads the parked column -- against a direct
//     evaluation of the shape over the dense matrix, bit for bit, on tests/track_rows.py's hostile w and amp values, with the slot
//     limit between a partial's w and amp slot, inside a group, at 0 and past the end, and with fewer staged rows than the limit;
//   * plan_stream, stream_launch and stream_launch_check: served with the option on, every refusal with its sentence, 65536 staged
//     rows served and 65537 refused, every checked field of the two new kernels' arguments broken in turn, the unnamed enum values.
// Stand-alone: built with graph.cpp, match.cpp, stage.cpp and leafjit.cpp and run on the CPU with -fsanitize=address,undefined by
// tests/test_stream_tracks_host.py.
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../libfriendship_amd/csrc/jit.hpp"
#include "streamplans.hpp"

static const char *const OLD_TRACKS = "these compiled voices read per-leaf track rows (track voices); block streaming interprets leaves over constants and streamed input rows only";
static const char *const OLD_LEAF = "a leaf reads a per-leaf track row (a track voice); block streaming interprets leaves over constants and streamed input rows only";
static const char *const OLD_TEMPLATE = "block streaming needs balanced template voices (these are general, compiled or track voices)";

// ---- graphs (as streamleaves_tests.cpp) ---------------------------------------------------------------------------------------
struct Operand { int kind; uint32_t v; };   // 0 = node handle, 1 = constant bits, 2 = input slot
static Operand N(uint32_t h) { return {0, h}; }
static Operand Cf(float f) { return {1, f32_to_bits(f)}; }
static Operand In(uint32_t s) { return {2, s}; }
struct Build {
    std::vector<std::pair<uint32_t, int>> nodes{{1, FR_PRIM_F32CONSTANT}};
    std::vector<fr_edge> edges;
    uint32_t next = 2;
    uint32_t op(int kind, Operand a, Operand b) {
        const uint32_t h = next++;
        nodes.push_back({h, kind});
        const Operand ops[2] = {a, b};
        for (uint32_t s = 0; s < 2; ++s) {
            if (ops[s].kind == 0) edges.push_back({ops[s].v, h, 0, s});
            else if (ops[s].kind == 1) edges.push_back({1, h, ops[s].v, s});
            else edges.push_back({0, h, ops[s].v, s});
        }
        return h;
    }
    void out(uint32_t h, uint32_t slot) { edges.push_back({h, 0, 0, slot}); }
    void apply(Mirror &m) const {
        for (auto &n : nodes) { fr_effect e{}; e.kind = n.second; m.add_node(n.first, &e); }
        for (auto &e : edges) m.add_edge(e);
    }
};
static uint32_t sum_tree(Build &b, std::vector<uint32_t> cur) {
    while (cur.size() > 1) {
        std::vector<uint32_t> nx;
        for (size_t i = 0; i + 1 < cur.size(); i += 2) nx.push_back(b.op(FR_PRIM_SUM2, N(cur[i]), N(cur[i + 1])));
        cur = nx;
    }
    return cur[0];
}
// libfriendship_amd/synth.py track_leaves: the 11-node partial oscillator, its phase increment and amplitude read from input rows
static uint32_t track_leaf(Build &b, uint32_t w_slot, uint32_t amp_slot) {
    const uint32_t ph = b.op(FR_PRIM_MODULO, N(b.op(FR_PRIM_MULTIPLY, In(0), In(w_slot))), Cf(1.0f));
    const uint32_t u = b.op(FR_PRIM_SUM2, N(ph), Cf(-0.5f));
    const uint32_t m = b.op(FR_PRIM_MINIMUM, N(u), N(b.op(FR_PRIM_MULTIPLY, Cf(-1.0f), N(u))));
    const uint32_t n1 = b.op(FR_PRIM_MULTIPLY, Cf(-1.0f), N(b.op(FR_PRIM_MULTIPLY, Cf(-1.0f), N(m))));
    const uint32_t q = b.op(FR_PRIM_SUM2, Cf(0.5f), N(n1));
    const uint32_t y = b.op(FR_PRIM_MULTIPLY, N(b.op(FR_PRIM_MULTIPLY, Cf(-16.0f), N(u))), N(q));
    return b.op(FR_PRIM_MULTIPLY, In(amp_slot), N(y));
}
using LeafFn = std::function<uint32_t(Build &, uint32_t voice, uint32_t k)>;
// synth.track_tree: slot first + 2 (v P + k) holds w, the next one amp
static LeafFn tree_leaf(uint32_t P, uint32_t first = 1) {
    return [P, first](Build &b, uint32_t v, uint32_t k) { return track_leaf(b, first + 2 * (v * P + k), first + 2 * (v * P + k) + 1); };
}

struct Planned {
    FlatGraph fg;
    StagedPlan sp;
    std::vector<BankLaunch> banks;
    StreamEnv env;
    std::vector<const BankLaunch *> list() const {
        std::vector<const BankLaunch *> l;
        for (const BankLaunch &b : banks) l.push_back(&b);
        return l;
    }
    StreamPlan plan() const { return plan_stream(sp, list(), env); }
};
static Planned planned(const std::vector<std::pair<uint32_t, LeafFn>> &voices, uint32_t track_from = 1) {
    Build b;
    for (uint32_t v = 0; v < voices.size(); ++v) {
        std::vector<uint32_t> leaves;
        for (uint32_t k = 0; k < voices[v].first; ++k) leaves.push_back(voices[v].second(b, v, k));
        b.out(sum_tree(b, leaves), v);
    }
    Mirror m;
    b.apply(m);
    Planned p;
    p.fg = lower(m, (uint32_t)voices.size());
    p.sp = plan_stages(p.fg, true, true, 20, /*allow_jit=*/true, true, nullptr, nullptr, track_from);
    p.banks = std::move(p.sp.banks);
    p.env.n_slots = (uint32_t)voices.size();
    p.env.programs = p.env.leaves = p.env.tracks = true;
    p.env.track_from = track_from;
    return p;
}

// ---- the compiler -----------------------------------------------------------------------------------------------------------
static bool program_well_formed(const LeafProgram &lp) {
    bool ok = lp.ins.size() <= LEAF_PROG_MAX_INSTRS && lp.regs <= LEAF_PROG_MAX_REGS && lp.k >= 1 && lp.track_cols.size() <= LEAF_PROG_MAX_TRACKS;
    std::vector<bool> written(LEAF_PROG_MAX_REGS, false);
    auto operand_ok = [&](uint32_t kind, uint32_t v) {
        if (kind == LEAF_REG) return v < lp.regs && written[v];
        if (kind == LEAF_PARAM) return v < lp.k;
        if (kind == LEAF_IN) return v < lp.input_slots.size();
        if (kind == LEAF_TRK) return v < lp.k && lp.track_index(kind, v) < lp.track_cols.size();
        if (kind == LEAF_TRK_LIT) return lp.track_index(kind, v) < lp.track_cols.size();
        return kind == LEAF_LIT;
    };
    for (const LeafInstr &in : lp.ins) {
        ok = ok && in.op >= LEAF_OP_SUM2 && in.op <= LEAF_OP_MIN && in.dst < lp.regs && in.ka < 8 && in.kb < 8 && operand_ok(in.ka, in.a) && operand_ok(in.kb, in.b);
        if (!ok) return false;
        written[in.dst] = true;
    }
    for (size_t i = 0; i < lp.track_cols.size(); ++i)
        for (size_t j = 0; j < i; ++j) ok = ok && !(lp.track_cols[i] == lp.track_cols[j]);   // distinct
    return ok;
}
static auto cols(uint32_t n, bool vary) { return std::vector<bool>(n, vary); }
static std::vector<uint32_t> ident(uint32_t n) { std::vector<uint32_t> a(n); for (uint32_t i = 0; i < n; ++i) a[i] = i; return a; }
// in0 * track(c0) * track(c1) ...: n track operands over n constant columns
static LeafShape track_chain(uint32_t n) {
    LeafShape s;
    s.input_slots = {0};
    s.n_consts = n;
    s.ops.push_back({OP_INPUT, 0, 0});
    for (uint32_t i = 0; i < n; ++i) {
        s.ops.push_back({LEAF_TRACK, i, 0});
        s.ops.push_back({OP_MUL, (uint32_t)s.ops.size() - 2u, (uint32_t)s.ops.size() - 1u});
    }
    return s;
}

static void test_compiler() {
    {   // synth.track_tree's leaf as BankMatcher makes it
        Planned p = planned({{128, tree_leaf(128)}});
        CHECK(p.banks.size() == 1 && p.banks[0].jit && p.banks[0].tracks && p.banks[0].log2_p == 7 && p.banks[0].max_track_slot == 256);
        const BankLaunch &b = p.banks[0];
        LeafProgram lp;
        std::string why;
        CHECK(!compile_leaf_program(b.shape, b.varying, b.literal_bits, b.alias, lp, &why) && why == OLD_LEAF);
        CHECK(!compile_leaf_program(b.shape, b.varying, b.literal_bits, b.alias, lp, &why, false) && why == OLD_LEAF && lp.track_cols.empty());
        why.clear();
        CHECK(compile_leaf_program(b.shape, b.varying, b.literal_bits, b.alias, lp, &why, true) && why.empty() && program_well_formed(lp));
        CHECK(lp.ins.size() <= 32 && lp.ins.size() >= 11 && lp.regs <= 8 && lp.track_cols.size() == 2 && lp.k == std::max(b.k, 1u) && lp.k == 2);
        CHECK(!lp.track_cols[0].literal && !lp.track_cols[1].literal && lp.track_cols[0].v != lp.track_cols[1].v && lp.input_slots == std::vector<uint32_t>{0});
        uint32_t trk = 0, params = 0;
        for (const LeafInstr &in : lp.ins) { trk += (in.ka == LEAF_TRK) + (in.kb == LEAF_TRK); params += (in.ka == LEAF_PARAM) + (in.kb == LEAF_PARAM); }
        CHECK(trk >= 2 && params == 0);          // every parameter column of this leaf holds a slot number
        // the table holds the slot numbers as bits: partial i reads slots 1 + 2 i and 2 + 2 i
        const uint32_t wc = lp.ins[0].ka == LEAF_TRK ? lp.ins[0].a : lp.ins[0].b;
        CHECK(f32_to_bits(b.params[5 * 2 + wc]) == 1 + 2 * 5 && f32_to_bits(b.params[5 * 2 + (1 - wc)]) == 2 + 2 * 5);
    }
    {   // 4 track operands fit, 5 are refused with the count and the limit
        LeafProgram lp;
        std::string why;
        CHECK(compile_leaf_program(track_chain(4), cols(4, true), std::vector<uint32_t>(4, 0), ident(4), lp, &why, true) && lp.track_cols.size() == 4 && lp.k == 4 && program_well_formed(lp));
        CHECK(!compile_leaf_program(track_chain(5), cols(5, true), std::vector<uint32_t>(5, 0), ident(5), lp, &why, true));
        CHECK(why == "a leaf that reads 5 distinct track rows; block streaming interprets leaves with at most 4");
        CHECK(!compile_leaf_program(track_chain(5), cols(5, true), std::vector<uint32_t>(5, 0), ident(5), lp, &why) && why == OLD_LEAF);
    }
    {   // 5 operands over aliased columns: columns 1..4 alias column 0 -- one track column, one parameter
        LeafProgram lp;
        CHECK(compile_leaf_program(track_chain(5), cols(5, true), std::vector<uint32_t>(5, 0), std::vector<uint32_t>(5, 0), lp, nullptr, true));
        CHECK(lp.track_cols.size() == 1 && lp.k == 1 && lp.ins.size() == 5 && program_well_formed(lp));
        for (const LeafInstr &in : lp.ins) CHECK(in.kb == LEAF_TRK && in.b == 0);
    }
    {   // a literal slot: the column does not vary; next to a varying one; the same literal twice is one column
        LeafProgram lp;
        CHECK(compile_leaf_program(track_chain(3), {false, true, false}, {7, 0, 7}, ident(3), lp, nullptr, true) && program_well_formed(lp));
        CHECK(lp.track_cols.size() == 2 && lp.k == 1 && lp.track_cols[0].literal && lp.track_cols[0].v == 7 && !lp.track_cols[1].literal && lp.track_cols[1].v == 0);
        CHECK(lp.ins[0].kb == LEAF_TRK_LIT && lp.ins[0].b == 7 && lp.ins[1].kb == LEAF_TRK && lp.ins[2].kb == LEAF_TRK_LIT && lp.track_index(LEAF_TRK_LIT, 7) == 0);
    }
    {   // a leaf that is a bare track
        LeafShape s;
        s.n_consts = 1;
        s.ops = {{LEAF_TRACK, 0, 0}};
        LeafProgram lp;
        CHECK(compile_leaf_program(s, cols(1, true), {0}, {0}, lp, nullptr, true) && lp.ins.empty() && lp.result_kind == LEAF_TRK && lp.result == 0 && lp.track_cols.size() == 1);
    }
}

// ---- the model --------------------------------------------------------------------------------------------------------------
static float prim_mod(float a, float b) { const float rem = std::fmod(a, b); return rem < 0.0f ? rem + b : rem; }
static float prim_min(float a, float b, bool sparkle) { if (sparkle && a != a) return a; return (a < b || b != b) ? a : b; }
static float binop(uint32_t op, float a, float b, bool sparkle) {
    switch (op) {
    case OP_SUM2: return a + b;
    case OP_MUL: return a * b;
    case OP_DIV: return a / b;
    case OP_MOD: return prim_mod(a, b);
    default: return prim_min(a, b, sparkle);
    }
}
static bool same(float a, float b) { return f32_to_bits(a) == f32_to_bits(b) || (a != a && b != b); }
// One frame of a block: the dense matrix's column (by slot), the first track slot and the limit the dense call gives jit_track.
struct Frame {
    std::vector<float> column;       // [slot]: the matrix's value at this frame
    uint32_t first_slot, limit;
    float track(uint32_t slot) const { return slot < limit && slot < column.size() ? column[slot] : 0.0f; }   // jit_track
};
// the shape's ops, directly (leafjit.cpp's reading of LEAF_TRACK: the slot is the column's bits)
static float eval_shape(const LeafShape &s, const std::vector<uint32_t> &consts, const Frame &f, bool sparkle) {
    std::vector<float> v(s.ops.size());
    for (size_t i = 0; i < s.ops.size(); ++i) {
        const LeafShape::Op &o = s.ops[i];
        v[i] = o.op == OP_CONST ? f32_from_bits(consts[o.a]) : o.op == OP_INPUT ? f.column[s.input_slots[o.a]] : o.op == LEAF_TRACK ? f.track(consts[o.a])
                                                                                                                                  : binop(o.op, v[o.a], v[o.b], sparkle);
    }
    return v.back();
}
static float sum_rec(const std::vector<float> &l, size_t lo, size_t n) { return n == 1 ? l[lo] : sum_rec(l, lo, n / 2) + sum_rec(l, lo + n / 2, n / 2); }

// kernels.hip StreamTrackWave / stream_render_leaves<true> for one frame.  `staging`: [staged rows] the host's copy of the block
// (rows first_slot ..); `alloc_rows`: what the launch holds; `block_rows`, `limit`: the control word.
static float model_voice(const LeafProgram &lp, const std::vector<float> &params, uint32_t log2_p, uint32_t chunk_log2, const Frame &f, const std::vector<float> &staging,
                         uint32_t alloc_rows, uint32_t block_rows, bool sparkle, uint64_t &parks) {
    const uint32_t nchunks = 1u << (log2_p - chunk_log2), Pw = (1u << chunk_log2) / 16u, NT = (uint32_t)lp.track_cols.size();
    auto counter = [](std::vector<float> &c, uint32_t j, float v) {
        uint32_t k = 0;
        for (; (j >> k) & 1u; ++k) v = c[k] + v;
        c[k] = v;
    };
    auto log2u = [](uint32_t n) { uint32_t l = 0; while ((1u << l) < n) ++l; return l; };
    auto slot_of = [&](uint32_t q, const float *prow) { return lp.track_cols[q].literal ? lp.track_cols[q].v : f32_to_bits(prow[lp.track_cols[q].v]); };
    auto load = [&](uint32_t q, const float *prow) {          // the load: in bounds of the allocation, whatever the block says
        if (q >= NT) return 0.0f;
        const uint32_t off = slot_of(q, prow) - f.first_slot;
        return off < alloc_rows && off < staging.size() ? staging[off] : 0.0f;
    };
    std::vector<float> chunk_carry(10, 0.0f);
    for (uint32_t chunk = 0; chunk < nchunks; ++chunk) {
        float sm[16];
        for (uint32_t wave = 0; wave < 16; ++wave) {
            float regs[LEAF_PROG_MAX_REGS] = {};
            float park[2][LEAF_PROG_MAX_TRACKS] = {{NAN, NAN, NAN, NAN}, {NAN, NAN, NAN, NAN}};   // (a read of the wrong half shows)
            const float *prow = params.data() + ((size_t)(chunk << chunk_log2) + (size_t)wave * Pw) * lp.k;
            float next[LEAF_PROG_MAX_TRACKS];
            for (uint32_t q = 0; q < LEAF_PROG_MAX_TRACKS; ++q) next[q] = load(q, prow);
            std::vector<float> c(12, 0.0f);
            for (uint32_t j = 0; j < Pw; ++j, prow += lp.k) {
                float *tp = park[j & 1u];
                for (uint32_t q = 0; q < NT; ++q) {            // the park: the block's limit and staged rows
                    const uint32_t s = slot_of(q, prow);
                    tp[q] = s < f.limit && s - f.first_slot < block_rows ? next[q] : 0.0f;
                    ++parks;
                }
                if (j + 1 < Pw)
                    for (uint32_t q = 0; q < LEAF_PROG_MAX_TRACKS; ++q) next[q] = load(q, prow + lp.k);
                auto operand = [&](uint32_t kind, uint32_t v) {
                    if (kind == LEAF_TRK || kind == LEAF_TRK_LIT) return tp[lp.track_index(kind, v) & 3u];   // (the upload's rewrite: v = the place)
                    return kind == LEAF_REG ? regs[v & 7u] : kind == LEAF_PARAM ? prow[v] : kind == LEAF_LIT ? f32_from_bits(v) : f.column[lp.input_slots[v]];
                };
                float v = 0.0f;
                for (const LeafInstr &in : lp.ins) {
                    v = binop(in.op, operand(in.ka, in.a), operand(in.kb, in.b), sparkle);
                    regs[in.dst & 7u] = v;
                }
                counter(c, j, lp.result_kind == LEAF_REG ? v : operand(lp.result_kind, lp.result));
                tp[0] = tp[1] = tp[2] = tp[3] = NAN;           // (the next use of this half must park first)
            }
            sm[wave] = c[log2u(Pw)];
        }
        for (uint32_t n = 8; n >= 1; n /= 2)
            for (uint32_t i = 0; i < n; ++i) sm[i] = sm[2 * i] + sm[2 * i + 1];
        if (nchunks == 1) return sm[0];
        counter(chunk_carry, chunk, sm[0]);
    }
    return chunk_carry[log2u(nchunks)];
}

// tests/track_rows.py
static const float HOSTILE_W[] = {-0.013f, -0.0f, NAN, INFINITY, -INFINITY, 1e30f, 1e-45f, -3e-39f, 1.0f, 0.5f, 16.0f, -2.0f, 3e38f, 0.25f, -1e-30f, 8.0f, 0.0f};
static const float HOSTILE_AMP[] = {0.0f, -0.0f, -0.7f, NAN, INFINITY, -INFINITY, 1e-45f, -3e-39f, 3e38f, -1.0f, 0.0f, -0.0f, 2.5f};

static void test_model() {
    uint64_t compared = 0, parks = 0;
    for (uint32_t log2_p : {7u, 8u, 9u}) {
        const uint32_t P = 1u << log2_p, first = 1, slots = first + 2 * P;
        Planned p = planned({{P, tree_leaf(P)}});
        CHECK(p.banks.size() == 1 && p.banks[0].jit && p.banks[0].tracks && p.banks[0].log2_p == log2_p);
        if (p.banks.size() != 1 || !p.banks[0].tracks) continue;
        const BankLaunch &b = p.banks[0];
        LeafProgram lp;
        CHECK(compile_leaf_program(b.shape, b.varying, b.literal_bits, b.alias, lp, nullptr, true));
        // every leaf's own column values: a varying column from the table, any other its literal
        std::vector<std::vector<uint32_t>> consts(P, std::vector<uint32_t>(b.shape.n_consts));
        for (uint32_t i = 0; i < P; ++i) {
            uint32_t j = 0;
            std::vector<uint32_t> col_param(b.shape.n_consts, 0);
            for (uint32_t c = 0; c < b.shape.n_consts; ++c) {
                if (b.varying[c] && b.alias[c] == c) col_param[c] = j++;
                consts[i][c] = !b.varying[c] ? b.literal_bits[c] : f32_to_bits(b.params[(size_t)i * lp.k + col_param[b.alias[c]]]);
            }
        }
        // the limits: past the end, between partial 9's w and amp slot, inside a group (partial 3's w slot), at 0, one row
        const uint32_t limits[] = {slots + 5, slots, first + 2 * 9 + 1, first + 2 * 3, 0, first + 1};
        for (int sparkle = 0; sparkle < 2; ++sparkle)
            for (uint32_t frame = 0; frame < 12; ++frame)
                for (uint32_t limit : limits) {
                    Frame f;
                    f.first_slot = first;
                    f.limit = limit;
                    f.column.assign(slots, 0.0f);
                    f.column[0] = frame == 3 ? -0.75f : frame == 7 ? NAN : (float)((1u << 20) + 37 + frame);
                    for (uint32_t k = 0; k < P; ++k) {
                        const bool hostile = frame < 8 && (k < 8 || k >= P - 8 || (k >= P / 16 && k < P / 8));   // the first and last group, one wave's share
                        f.column[first + 2 * k] = hostile ? HOSTILE_W[(k + 3 * frame) % 17] : 0.0007f * (float)(k + 1) + 1e-5f * (float)frame;
                        f.column[first + 2 * k + 1] = hostile ? HOSTILE_AMP[(5 * k + frame) % 13] : (0.5f + 0.1f * (float)frame) / (float)(k + 1);
                    }
                    std::vector<float> leaves(P);
                    for (uint32_t i = 0; i < P; ++i) leaves[i] = eval_shape(b.shape, consts[i], f, sparkle != 0);
                    const float expect = sum_rec(leaves, 0, P);
                    // the host's staging: the rows below the limit, from the first track slot (engine.cpp stream_block_rows); what lies
                    // beyond is the previous block's -- poison here
                    const uint32_t alloc = b.max_track_slot - first + 1, staged = limit > first ? std::min(limit - first, alloc) : 0;
                    CHECK(alloc == 2 * P);
                    std::vector<float> staging(alloc, 12345.0f);
                    for (uint32_t q = 0; q < staged; ++q) staging[q] = f.column[first + q];
                    for (uint32_t chunk_log2 : {7u, 8u, 9u}) {
                        if (chunk_log2 > log2_p) continue;
                        const float got = model_voice(lp, b.params, log2_p, chunk_log2, f, staging, alloc, staged, sparkle != 0, parks);
                        CHECK(same(got, expect));
                        ++compared;
                    }
                    if (limit == 0 || limit == first + 1) CHECK(same(expect, 0.0f) || expect != expect);   // every track +0: amp 0 times a finite or NaN wave
                }
    }
    CHECK(compared == 2u * 12 * 6 * (1 + 2 + 3) && parks > 0);
    {   // a literal slot next to a per-partial one, and the limit below the literal's slot
        LeafProgram lp;
        CHECK(compile_leaf_program(track_chain(2), {true, false}, {0, 4}, ident(2), lp, nullptr, true));
        std::vector<float> params(128);
        for (uint32_t i = 0; i < 128; ++i) params[i] = f32_from_bits(2 + (i % 3));
        for (uint32_t limit : {6u, 4u, 3u, 0u}) {
            Frame f{{2.0f, 9.0f, 3.0f, 5.0f, 7.0f, 11.0f}, 2, limit};
            std::vector<float> leaves(128);
            for (uint32_t i = 0; i < 128; ++i) leaves[i] = f.column[0] * f.track(2 + (i % 3)) * f.track(4);
            const uint32_t staged = limit > 2 ? limit - 2 : 0;
            std::vector<float> staging(4, 777.0f);
            for (uint32_t q = 0; q < staged; ++q) staging[q] = f.column[2 + q];
            CHECK(same(model_voice(lp, params, 7, 7, f, staging, 4, staged, false, parks), sum_rec(leaves, 0, 128)));
        }
    }
}

// ---- the rules --------------------------------------------------------------------------------------------------------------
static void test_serving_rule() {
    {   // served with the option on; each prerequisite missing in turn: the parent's sentence
        Planned p = planned({{128, tree_leaf(128)}, {128, tree_leaf(128)}});
        CHECK(p.banks.size() == 1 && p.banks[0].jit && p.banks[0].tracks && p.banks[0].rows.size() == 2 && p.sp.progs.empty() && p.banks[0].max_track_slot == 512);
        CHECK(stream_path(p.sp, p.list(), p.env));
        StreamPlan s = p.plan();
        CHECK(s.servable && s.reason.empty() && s.voices == 2 && s.banks.size() == 1 && s.banks[0].leaf && s.has_leaves() && s.has_tracks());
        CHECK(s.track_first == 1 && s.track_rows == 512 && s.leaf_progs.size() == 1 && s.leaf_progs[0].track_cols.size() == 2 && s.input_slots == std::vector<uint32_t>{0});
        CHECK(s.workgroups() == 2 && s.banks[0].chunk_log2 == 7);
        Planned off = p;
        off.env.tracks = false;
        StreamPlan t = off.plan();
        CHECK(!t.servable && t.reason == OLD_TRACKS && !t.has_tracks() && t.track_rows == 0 && t.leaf_progs.empty());
        off = p;
        off.env.leaves = false;                 // FR_STREAM_TRACKS does nothing without FR_STREAM_LEAVES ...
        CHECK(off.plan().reason == OLD_TEMPLATE && !off.plan().has_tracks());
        off = p;
        off.env.programs = false;               // ... or without FR_STREAM_PROGRAMS
        CHECK(!stream_path(off.sp, off.list(), off.env) && off.plan().reason == OLD_TEMPLATE);
    }
    {   // chunks, as a template bank is dealt
        Planned p = planned({{512, tree_leaf(512)}, {512, tree_leaf(512)}});
        StreamPlan s = p.plan();
        CHECK(s.servable && s.banks[0].leaf && s.banks[0].chunk_log2 == 7 && s.chunks == 4 && s.workgroups() == 8 && s.track_rows == 2048);
    }
    {   // a track history, in each of its three signs
        Planned p = planned({{128, tree_leaf(128)}});
        Planned h = p;
        h.env.track_history = true;
        CHECK(h.plan().reason == "block streaming with a track history");
        h = p;
        h.sp.track_lookback = 3;
        CHECK(h.plan().reason == "block streaming with a track history");
        h = p;
        h.sp.track_window_slots.push_back(5);
        CHECK(h.plan().reason == "block streaming with a track history");
    }
    {   // 32 and 64 partials; a chunked compiled bank over a workspace; a sweep plan
        for (uint32_t P : {64u, 32u}) {
            Planned p = planned({{P, tree_leaf(P)}});
            CHECK(p.banks.size() == 1 && p.banks[0].tracks);
            CHECK(p.plan().reason == "compiled voices of " + std::to_string(P) + " partials; block streaming interprets the leaves of voices of at least 128 partials (16 waves x one group of 8)");
        }
        Planned p = planned({{128, tree_leaf(128)}});
        Planned ws = p;
        ws.banks[0].to_ws = true;
        CHECK(ws.plan().reason == "a compiled bank that is cut into chunks over an exchange workspace; block streaming serves whole compiled voices only");
        Planned sweep = p;
        sweep.sp.fused_sweep = 4;
        sweep.env.loops = sweep.env.dyn = sweep.env.sweep = true;
        CHECK(sweep.plan().reason == "a sweep plan (a feedback loop that delays by a signal amount) together with compiled voices; block streaming has no sweep form with a leaf interpreter");
    }
    {   // a leaf with 5 track rows: the count and the limit (the matched shape extended by hand)
        Planned p = planned({{128, tree_leaf(128)}});
        BankLaunch &b = p.banks[0];
        for (uint32_t extra = 0; extra < 3; ++extra) {
            b.shape.ops.push_back({LEAF_TRACK, b.shape.n_consts, 0});
            b.shape.ops.push_back({OP_MUL, (uint32_t)b.shape.ops.size() - 2u, (uint32_t)b.shape.ops.size() - 1u});
            ++b.shape.n_consts;
            b.varying.push_back(true);
            b.literal_bits.push_back(0);
            b.alias.push_back(b.shape.n_consts - 1);
        }
        CHECK(p.plan().reason == "a leaf that reads 5 distinct track rows; block streaming interprets leaves with at most 4");
    }
    {   // the staging cap: 65536 rows served, 65537 refused with the count and the limit
        Planned p = planned({{128, tree_leaf(128)}});
        p.banks[0].max_track_slot = 65536;      // slots 1 .. 65536
        StreamPlan s = p.plan();
        CHECK(s.servable && s.track_rows == 65536 && s.track_rows == STREAM_MAX_TRACK_ROWS);
        p.banks[0].max_track_slot = 65537;
        s = p.plan();
        CHECK(!s.servable && s.reason == "these track voices name 65537 track rows (slots 1 .. 65537); block streaming stages at most 65536 per block" && !s.has_tracks());
        // 256 workgroups x 128 partials x 2 rows is the cap
        CHECK(256u * 128u * 2u == STREAM_MAX_TRACK_ROWS && (size_t)STREAM_MAX_TRACK_ROWS * 64 * sizeof(float) == (16u << 20));
    }
    {   // a track bank next to a template bank needs FR_STREAM_BANKS like any second bank; a control row needs FR_STREAM_INPUTS
        Planned p = planned({{128, [](Build &b, uint32_t, uint32_t k) { return b.op(FR_PRIM_MULTIPLY, In(1), N(track_leaf(b, 2 + 2 * k, 3 + 2 * k))); }}}, 2);
        CHECK(p.banks.size() == 1 && p.banks[0].tracks);
        CHECK(p.plan().reason == "a leaf reads input slot 1; block streaming feeds slot 0 only");
        p.env.inputs = true;
        StreamPlan s = p.plan();
        CHECK(s.servable && s.input_slots == (std::vector<uint32_t>{0, 1}) && s.track_first == 2 && s.track_rows == 256 && stream_launch(p.sp, s).n_rows == 2);
    }
    {   // plans without a track bank are what they were, with the option on or off
        for (StreamKernel k : {StreamKernel::prog, StreamKernel::bus, StreamKernel::in, StreamKernel::banks, StreamKernel::loops, StreamKernel::general, StreamKernel::dyn}) {
            Built b = kernel_plan(k);
            const StreamPlan off = b.plan();
            b.env.leaves = b.env.tracks = true;
            const StreamPlan on = b.plan();
            CHECK(on.servable && off.servable && !on.has_tracks() && on.track_rows == 0 && stream_launch(b.sp, on).kernel == k && stream_launch(b.sp, off).kernel == k);
            CHECK(on.progs == off.progs && on.voice_first == off.voice_first && on.input_slots == off.input_slots && on.workgroups() == off.workgroups());
        }
    }
}

static void test_launch_rule_and_check() {
    CHECK((uint32_t)StreamKernel::track == (uint32_t)StreamKernel::leaf_store + 2 && (uint32_t)StreamKernel::track_store == (uint32_t)StreamKernel::track + 2);
    for (uint32_t d : {1u, 3u, 5u}) CHECK(!stream_kernel_named((StreamKernel)((uint32_t)StreamKernel::leaf_store + d)));
    CHECK(stream_kernel_named(StreamKernel::track) && stream_kernel_named(StreamKernel::track_store));
    CHECK(std::string(stream_kernel_name(StreamKernel::track)) == "bank_stream_track_kernel" && std::string(stream_kernel_name(StreamKernel::track_store)) == "bank_stream_track_store_kernel");
    {   // the forms: the leaf forms, and the flag
        const StreamForm t = stream_form(StreamKernel::track), l = stream_form(StreamKernel::leaf), ts = stream_form(StreamKernel::track_store), ls = stream_form(StreamKernel::leaf_store);
        CHECK(t.tracks && ts.tracks && t.leaf && ts.leaf && !t.store && ts.store && !t.sweep && !t.voiceless);
        CHECK(t.progs == l.progs && t.bus == l.bus && t.rows == l.rows && t.table == l.table && t.loops == l.loops && t.schedule == l.schedule && t.dyn == l.dyn && t.hist == l.hist);
        CHECK(ts.progs == ls.progs && ts.table == ls.table && ts.loops == ls.loops && ts.schedule == ls.schedule && ts.dyn == ls.dyn && ts.hist == ls.hist);
        for (StreamKernel k : {StreamKernel::plain, StreamKernel::prog, StreamKernel::bus, StreamKernel::in, StreamKernel::banks, StreamKernel::loops, StreamKernel::general,
                               StreamKernel::dyn, StreamKernel::hist, StreamKernel::fx, StreamKernel::store, StreamKernel::store_fx, StreamKernel::sweep, StreamKernel::sweep_fx,
                               StreamKernel::sweep_store, StreamKernel::sweep_store_fx, StreamKernel::leaf, StreamKernel::leaf_store})
            CHECK(!stream_form(k).tracks);
    }
    Planned p = planned({{256, tree_leaf(256)}, {256, tree_leaf(256)}});
    p.env.device_cus = 256;
    StreamPlan s = p.plan();
    CHECK(s.servable && s.has_tracks());
    StreamLaunch l = stream_launch(p.sp, s);
    CHECK(l.kernel == StreamKernel::track && l.rows_doorbell && l.own_instrs && l.by_plan && l.bank_table && !l.schedule_table && l.n_rows == 1 && l.hist_cap == 64 && l.workgroups == 4);
    Planned st = p;
    st.env.store = true;
    CHECK(stream_launch(st.sp, st.plan()).kernel == StreamKernel::track_store && stream_launch(st.sp, st.plan()).hist_cap == 64);
    Planned notrk = planned({{256, [](Build &b, uint32_t, uint32_t k) { return b.op(FR_PRIM_MULTIPLY, Cf(1.0f / (float)(k + 1)), N(b.op(FR_PRIM_MODULO, N(b.op(FR_PRIM_MULTIPLY, In(0), Cf(0.001f * (float)(k + 1)))), Cf(1.0f)))); }}});
    CHECK(notrk.banks.size() == 1 && notrk.banks[0].jit && !notrk.banks[0].tracks && stream_launch(notrk.sp, notrk.plan()).kernel == StreamKernel::leaf);   // has_tracks() stands in front of has_leaves()

    // the launch check on the two new kernels' minimal arguments
    float dummy[4] = {};
    uint32_t words[4] = {};
    uint4 prog_words[13] = {};
    auto args = [&] {
        StreamLaunchArgs x{};
        x.a.leaf_variant = 1; x.a.out = dummy; x.a.n_voices = 2; x.a.ws = dummy; x.a.tickets = words;
        x.ctl_dev = dummy; x.dev = dummy; x.n_rows = 1;
        x.h.hist = dummy; x.h.mask = 63;
        x.p.voice_first = words;
        x.t.n_banks = 1;
        x.t.bank[0] = {(const float2 *)dummy, words, 0, 0, 2, 8, 7, 1, 0};
        x.l.mask = 1;
        x.l.bank[0] = {prog_words, 13, 2, LEAF_REG, 1};
        x.tr.staging = dummy; x.tr.first_slot = 1; x.tr.rows = 1024;
        x.tr.bank[0] = {2, 0, {0, 1, 0, 0}};
        return x;
    };
    for (StreamKernel k : {StreamKernel::track, StreamKernel::track_store}) {
        CHECK(stream_launch_check(k, args()) == 4);
        auto broken = [&](const std::function<void(StreamLaunchArgs &)> &f) { StreamLaunchArgs x = args(); f(x); return stream_launch_check(k, x) == 0; };
        CHECK(broken([](StreamLaunchArgs &x) { x.tr.staging = nullptr; }));                    // the staging pointer
        CHECK(broken([](StreamLaunchArgs &x) { x.tr.rows = 0; }));                             // ... and its row count
        CHECK(broken([](StreamLaunchArgs &x) { x.tr.rows = 65537; }));
        CHECK(!broken([](StreamLaunchArgs &x) { x.tr.rows = 65536; }));
        CHECK(broken([](StreamLaunchArgs &x) { x.tr.first_slot = 0xFFFFFFFFu; }));             // first_slot + rows past the slot numbers
        CHECK(broken([](StreamLaunchArgs &x) { x.tr.bank[0].n = 5; }));                        // the count <= 4
        CHECK(broken([](StreamLaunchArgs &x) { x.tr.bank[0].cols[1] = 2; }));                  // track_cols within k
        CHECK(!broken([](StreamLaunchArgs &x) { x.tr.bank[0].cols[1] = 2; x.tr.bank[0].literal = 2; }));   // (a literal slot is no column)
        CHECK(broken([](StreamLaunchArgs &x) { x.tr.bank[0].literal = 4; }));                  // a literal bit beyond the count
        CHECK(!broken([](StreamLaunchArgs &x) { x.tr.bank[0] = {}; }));                        // a leaf bank without a track next to one with (another bank's)
        CHECK(broken([](StreamLaunchArgs &x) { x.l.bank[0].result_kind = 4; x.l.bank[0].result = 2; }));   // a bare track the bank does not list
        CHECK(!broken([](StreamLaunchArgs &x) { x.l.bank[0].result_kind = 4; x.l.bank[0].result = 1; }));
        CHECK(broken([](StreamLaunchArgs &x) { x.l.bank[0].result_kind = 5; }));
        // the leaf form underneath
        CHECK(broken([](StreamLaunchArgs &x) { x.l.mask = 0; }));
        CHECK(broken([](StreamLaunchArgs &x) { x.l.bank[0].instrs = nullptr; }));
        CHECK(broken([](StreamLaunchArgs &x) { x.l.bank[0].n_instr = 33; }));
        CHECK(broken([](StreamLaunchArgs &x) { x.l.bank[0].k = 0; }));
        CHECK(broken([](StreamLaunchArgs &x) { x.t.bank[0].chunk_log2 = 6; }));
        CHECK(broken([](StreamLaunchArgs &x) { x.h.hist = nullptr; }));
        CHECK(broken([](StreamLaunchArgs &x) { x.n_rows = 9; }));
    }
    { StreamLaunchArgs x = args(); x.l.bank[0].result_kind = 4; x.l.bank[0].result = 0; CHECK(stream_launch_check(StreamKernel::leaf, x) == 0); }   // the leaf forms know no track
    { StreamLaunchArgs x = args(); x.tr = {}; CHECK(stream_launch_check(StreamKernel::leaf, x) == 4 && stream_launch_check(StreamKernel::track, x) == 0); }
    for (uint32_t d : {1u, 3u, 5u}) CHECK(stream_launch_check((StreamKernel)((uint32_t)StreamKernel::leaf_store + d), args()) == 0);
    CHECK(sizeof(BankStreamInCtl) == 8 * 64 * 8 + 64 && offsetof(BankStreamInCtl, tracks) == offsetof(BankStreamInCtl, alive) + 4);
}

int main() {
    test_compiler();
    test_model();
    test_serving_rule();
    test_launch_rule_and_check();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
