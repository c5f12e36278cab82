// streamleaves_tests.cpp -- FR_STREAM_LEAVES on the host (libfriendship_amd/csrc/leafprog.hpp, streamplan.hpp, kernels.hpp):
//   * the leaf-program compiler on matched and hand-built shapes: one instruction per arithmetic op, the register bound,
//     literal, varying and aliased columns, the refusals (a shape over either limit, a track leaf) with their sentences;
//   * a plain-loop model of kernels.hip stream_render_leaves -- 16 "waves" that each run the program per partial on their own
//     register columns and add the leaves with one binary counter, the wave sums in tree order, the chunk sums through the
//     hand-over's binary counter -- against a direct evaluation of the LeafShape's ops and a recursive balanced Sum2 tree written
//     here, bit for bit, P = 128, 256, 1024 in chunks of 128 / 256 / 1024, hostile inputs, both semantics;
//   * the serving rule, the launch rule and the launch check on plans that plan_stages(..., use_jit = true, ...) makes of real
//     graphs (a triangle voice and its kin): every new sentence, and each prerequisite option missing in turn.
// Stand-alone: built with graph.cpp, match.cpp, stage.cpp and leafjit.cpp and run on the CPU with -fsanitize=address,undefined by
// tests/test_stream_leaves_host.py.
#include <cmath>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "../../libfriendship_amd/csrc/jit.hpp"
#include "streamplans.hpp"

static const char *const OLD_TEMPLATE = "block streaming needs balanced template voices (these are general, compiled or track voices)";
static const char *const OLD_TEMPLATE_GENERAL = "block streaming needs template voices (these are compiled or track voices)";

// ---- graphs -----------------------------------------------------------------------------------------------------------------
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
// libfriendship_amd/synth.py triangle_leaves: amp * (1 - 4 * |Modulo(t * w, 1) - 0.5|), optionally times In(am)
static uint32_t triangle(Build &b, float w, float amp, int am = -1) {
    const uint32_t ph = b.op(FR_PRIM_MODULO, N(b.op(FR_PRIM_MULTIPLY, In(0), Cf(w))), Cf(1.0f));
    const uint32_t u = b.op(FR_PRIM_SUM2, N(ph), Cf(-0.5f));
    const uint32_t au = b.op(FR_PRIM_MULTIPLY, Cf(-1.0f), N(b.op(FR_PRIM_MINIMUM, N(u), N(b.op(FR_PRIM_MULTIPLY, Cf(-1.0f), N(u))))));
    const uint32_t tri = b.op(FR_PRIM_SUM2, Cf(1.0f), N(b.op(FR_PRIM_MULTIPLY, Cf(-4.0f), N(au))));
    const uint32_t leaf = b.op(FR_PRIM_MULTIPLY, Cf(amp), N(tri));
    return am < 0 ? leaf : b.op(FR_PRIM_MULTIPLY, N(leaf), In((uint32_t)am));
}
// Divide(Sum2(Modulo(Sum2(t * w, ph), 1), -0.5), d): three varying columns
static uint32_t saw_div(Build &b, float w, float ph, float d) {
    const uint32_t x = b.op(FR_PRIM_SUM2, N(b.op(FR_PRIM_MULTIPLY, In(0), Cf(w))), Cf(ph));
    return b.op(FR_PRIM_DIVIDE, N(b.op(FR_PRIM_SUM2, N(b.op(FR_PRIM_MODULO, N(x), Cf(1.0f))), Cf(-0.5f))), Cf(d));
}
using LeafFn = std::function<uint32_t(Build &, uint32_t voice, uint32_t k)>;
static LeafFn tri_leaf(int am = -1) {
    return [am](Build &b, uint32_t v, uint32_t k) { return triangle(b, 0.0011f * (float)(v + 1) * (float)(k + 1), 1.0f / (float)(k + 1), am); };
}

// A plan as the engine makes it of `voices` voices of P leaves each (one output row per voice), compiled banks included.
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
static Planned planned(const std::vector<std::pair<uint32_t, LeafFn>> &voices, uint32_t track_from = 0xFFFFFFFFu) {
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
    p.banks = std::move(p.sp.banks);             // (as the engine moves them out when it uploads them)
    p.env.n_slots = (uint32_t)voices.size();
    p.env.programs = true;
    p.env.leaves = true;
    return p;
}

// ---- the compiler -----------------------------------------------------------------------------------------------------------
static uint32_t arith_ops(const LeafShape &s) {
    uint32_t n = 0;
    for (const LeafShape::Op &o : s.ops) n += o.op >= OP_SUM2 && o.op <= OP_MIN ? 1u : 0u;
    return n;
}
static bool program_well_formed(const LeafProgram &lp) {
    bool ok = lp.ins.size() <= LEAF_PROG_MAX_INSTRS && lp.regs <= LEAF_PROG_MAX_REGS && lp.k >= 1;
    std::vector<bool> written(LEAF_PROG_MAX_REGS, false);
    for (const LeafInstr &in : lp.ins) {
        ok = ok && in.op >= LEAF_OP_SUM2 && in.op <= LEAF_OP_MIN && in.dst < lp.regs;
        for (int side = 0; side < 2; ++side) {
            const uint32_t kind = side ? in.kb : in.ka, v = side ? in.b : in.a;
            if (kind == LEAF_REG) ok = ok && v < lp.regs && written[v];   // a register is read after it was written
            if (kind == LEAF_PARAM) ok = ok && v < lp.k;
            if (kind == LEAF_IN) ok = ok && v < lp.input_slots.size();
        }
        if (!ok) return false;
        written[in.dst] = true;
    }
    if (lp.result_kind == LEAF_REG) ok = ok && !lp.ins.empty() && lp.result == lp.ins.back().dst;
    return ok;
}

static void test_compiler() {
    {   // the triangle: 12 ops in the tree form (u's three ops stand twice), two varying columns and the w column aliased
        Planned p = planned({{128, tri_leaf()}});
        CHECK(p.banks.size() == 1 && p.banks[0].jit && !p.banks[0].tracks && p.banks[0].log2_p == 7);
        const BankLaunch &b = p.banks[0];
        LeafProgram lp;
        std::string why;
        CHECK(compile_leaf_program(b.shape, b.varying, b.literal_bits, b.alias, lp, &why) && why.empty());
        CHECK(lp.ins.size() == arith_ops(b.shape) && lp.ins.size() == 12 && program_well_formed(lp));
        CHECK(lp.k == std::max(b.k, 1u) && lp.k == 2 && lp.k == generate_leaf_source(b.shape, b.varying, b.literal_bits, b.alias).k);
        CHECK(lp.regs >= 2 && lp.regs <= 4 && lp.input_slots == std::vector<uint32_t>{0} && lp.inputs_read == 1 && lp.result_kind == LEAF_REG);
        uint32_t params = 0, lits = 0, ins_in = 0, aliased = 0, w_col = 99, amp_col = 99;
        for (const LeafInstr &in : lp.ins)
            for (int side = 0; side < 2; ++side) {
                const uint32_t kind = side ? in.kb : in.ka, v = side ? in.b : in.a;
                params += kind == LEAF_PARAM; lits += kind == LEAF_LIT; ins_in += kind == LEAF_IN;
                if (kind == LEAF_PARAM && in.op == LEAF_OP_MUL && (side ? in.ka : in.kb) == LEAF_IN) { aliased += w_col == 99 || w_col == v ? 1u : 99u; w_col = v; }   // t * w: both copies read one column
                else if (kind == LEAF_PARAM) amp_col = v;
                if (kind == LEAF_LIT) CHECK(v == f32_to_bits(1.0f) || v == f32_to_bits(-0.5f) || v == f32_to_bits(-1.0f) || v == f32_to_bits(-4.0f));
            }
        CHECK(params == 3 && aliased == 2 && ins_in == 2 && lits == 8 && w_col < 2 && amp_col == 1 - w_col);
    }
    {   // all amplitudes equal: the column is a literal, one parameter is left
        Planned p = planned({{128, [](Build &b, uint32_t, uint32_t k) { return triangle(b, 0.0011f * (float)(k + 1), 0.75f); }}});
        CHECK(p.banks.size() == 1 && p.banks[0].jit);
        LeafProgram lp;
        CHECK(compile_leaf_program(p.banks[0].shape, p.banks[0].varying, p.banks[0].literal_bits, p.banks[0].alias, lp) && lp.k == 1 && program_well_formed(lp));
        bool amp_literal = false;
        for (const LeafInstr &in : lp.ins) amp_literal = amp_literal || (in.ka == LEAF_LIT && in.a == f32_to_bits(0.75f)) || (in.kb == LEAF_LIT && in.b == f32_to_bits(0.75f));
        CHECK(amp_literal);
    }
    {   // three varying columns; the leaf times a control row
        Planned p = planned({{128, [](Build &b, uint32_t, uint32_t k) { return saw_div(b, 0.0007f * (float)(k + 1), 0.01f * (float)k, 1.0f + (float)k); }}});
        LeafProgram lp;
        CHECK(p.banks.size() == 1 && p.banks[0].jit && compile_leaf_program(p.banks[0].shape, p.banks[0].varying, p.banks[0].literal_bits, p.banks[0].alias, lp));
        CHECK(lp.k == 3 && lp.ins.size() == 5 && lp.ins.back().op == LEAF_OP_DIV && program_well_formed(lp));
        Planned q = planned({{128, tri_leaf(1)}});
        CHECK(q.banks.size() == 1 && compile_leaf_program(q.banks[0].shape, q.banks[0].varying, q.banks[0].literal_bits, q.banks[0].alias, lp));
        CHECK(lp.ins.size() == 13 && lp.input_slots == (std::vector<uint32_t>{0, 1}) && lp.inputs_read == 2 && program_well_formed(lp));
    }
    // hand-built shapes
    auto chain = [](uint32_t n) {   // ((in0 * c0) + c1) + c2 ... : n arithmetic ops, one register
        LeafShape s;
        s.input_slots = {0};
        s.n_consts = n;
        s.ops.push_back({OP_INPUT, 0, 0});
        for (uint32_t i = 0; i < n; ++i) {
            s.ops.push_back({OP_CONST, i, 0});
            s.ops.push_back({i == 0 ? (uint32_t)OP_MUL : (uint32_t)OP_SUM2, (uint32_t)s.ops.size() - 2u, (uint32_t)s.ops.size() - 1u});
        }
        return s;
    };
    auto cols = [](uint32_t n, bool vary) { return std::vector<bool>(n, vary); };
    auto ident = [](uint32_t n) { std::vector<uint32_t> a(n); for (uint32_t i = 0; i < n; ++i) a[i] = i; return a; };
    {
        LeafProgram lp;
        std::string why;
        const LeafShape s32 = chain(32), s33 = chain(33);
        CHECK(compile_leaf_program(s32, cols(32, false), std::vector<uint32_t>(32, f32_to_bits(2.0f)), ident(32), lp, &why) && lp.ins.size() == 32 && lp.regs == 1 && lp.k == 1);
        CHECK(program_well_formed(lp));
        CHECK(!compile_leaf_program(s33, cols(33, false), std::vector<uint32_t>(33, f32_to_bits(2.0f)), ident(33), lp, &why));
        CHECK(why == "a leaf of 33 arithmetic ops; block streaming interprets leaves of at most 32");
    }
    for (uint32_t live : {8u, 9u}) {   // `live` products that all stay live, then their sums: `live` registers
        LeafShape s;
        s.input_slots = {0};
        s.n_consts = live;
        std::vector<uint32_t> prod;
        for (uint32_t i = 0; i < live; ++i) {
            s.ops.push_back({OP_INPUT, 0, 0});
            s.ops.push_back({OP_CONST, i, 0});
            s.ops.push_back({OP_MUL, (uint32_t)s.ops.size() - 2u, (uint32_t)s.ops.size() - 1u});
            prod.push_back((uint32_t)s.ops.size() - 1u);
        }
        uint32_t acc = prod[0];
        for (uint32_t i = 1; i < live; ++i) { s.ops.push_back({OP_SUM2, acc, prod[i]}); acc = (uint32_t)s.ops.size() - 1u; }
        LeafProgram lp;
        std::string why;
        const bool ok = compile_leaf_program(s, cols(live, true), std::vector<uint32_t>(live, 0), ident(live), lp, &why);
        CHECK(ok == (live == 8));
        if (ok) CHECK(lp.regs == 8 && lp.k == 8 && lp.ins.size() == 15 && program_well_formed(lp));
        else CHECK(why == "a leaf that needs 9 registers; block streaming interprets leaves with at most 8");
    }
    {   // a track leaf; a bare input
        LeafShape s;
        s.input_slots = {0};
        s.n_consts = 1;
        s.ops = {{OP_INPUT, 0, 0}, {LEAF_TRACK, 0, 0}, {OP_MUL, 0, 1}};
        LeafProgram lp;
        std::string why;
        CHECK(!compile_leaf_program(s, cols(1, true), {0}, {0}, lp, &why));
        CHECK(why == "a leaf reads a per-leaf track row (a track voice); block streaming interprets leaves over constants and streamed input rows only");
        s.ops = {{OP_INPUT, 0, 0}};
        s.n_consts = 0;
        CHECK(compile_leaf_program(s, {}, {}, {}, lp, &why) && lp.ins.empty() && lp.result_kind == LEAF_IN && lp.result == 0 && lp.k == 1 && lp.regs == 0);
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
// the shape's ops, directly: constants from the leaf's own column values (all columns, before any aliasing or literal folding)
static float eval_shape(const LeafShape &s, const std::vector<uint32_t> &consts, const std::vector<float> &in, bool sparkle) {
    std::vector<float> v(s.ops.size());
    for (size_t i = 0; i < s.ops.size(); ++i) {
        const LeafShape::Op &o = s.ops[i];
        v[i] = o.op == OP_CONST ? f32_from_bits(consts[o.a]) : o.op == OP_INPUT ? in[o.a] : binop(o.op, v[o.a], v[o.b], sparkle);
    }
    return v.back();
}
static float sum_rec(const std::vector<float> &l, size_t lo, size_t n) { return n == 1 ? l[lo] : sum_rec(l, lo, n / 2) + sum_rec(l, lo + n / 2, n / 2); }

// kernels.hip stream_leaf_operand / stream_leaf / stream_render_leaves / stream_hand_over for one frame: `params` [P][k], rows[r]
static float model_voice(const LeafProgram &lp, const std::vector<float> &params, uint32_t log2_p, uint32_t chunk_log2, const std::vector<float> &rows, bool sparkle) {
    const uint32_t nchunks = 1u << (log2_p - chunk_log2), Pw = (1u << chunk_log2) / 16u;
    auto counter = [](std::vector<float> &c, uint32_t j, float v) {   // the binary counter's step
        uint32_t k = 0;
        for (; (j >> k) & 1u; ++k) v = c[k] + v;
        c[k] = v;
    };
    auto log2u = [](uint32_t n) { uint32_t l = 0; while ((1u << l) < n) ++l; return l; };
    std::vector<float> chunk_carry(10, 0.0f);
    for (uint32_t chunk = 0; chunk < nchunks; ++chunk) {
        float sm[16];
        for (uint32_t wave = 0; wave < 16; ++wave) {
            float regs[LEAF_PROG_MAX_REGS] = {};
            const float *prow = params.data() + ((size_t)(chunk << chunk_log2) + (size_t)wave * Pw) * lp.k;
            std::vector<float> c(12, 0.0f);
            for (uint32_t j = 0; j < Pw; ++j, prow += lp.k) {
                auto operand = [&](uint32_t kind, uint32_t v) {
                    return kind == LEAF_REG ? regs[v & 7u] : kind == LEAF_PARAM ? prow[v] : kind == LEAF_LIT ? f32_from_bits(v) : rows[v & 7u];
                };
                float v = 0.0f;
                for (const LeafInstr &in : lp.ins) {
                    const float x = operand(in.ka, in.a), y = operand(in.kb, in.b);
                    v = binop(in.op, x, y, sparkle);
                    regs[in.dst & 7u] = v;
                }
                counter(c, j, lp.result_kind == LEAF_REG ? v : operand(lp.result_kind, lp.result));
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

static void test_model() {
    const float hostile[] = {0.0f, -0.0f, 1.0f, 0.5f, 0.25f, 3.0f, 1e-30f, 1e-42f, -1e-42f, 48000.0f, 16777216.0f, 4294967296.0f, 4294967808.0f,
                             1e30f, 3e38f, -1.0f, -0.5f, -2.75f, -48000.25f, -1e30f, INFINITY, -INFINITY, NAN};
    struct Case { const char *name; LeafFn leaf; uint32_t n_in; };
    const std::vector<Case> cases = {
        {"triangle", tri_leaf(), 1},
        {"triangle x in1", tri_leaf(1), 2},
        {"saw / d", [](Build &b, uint32_t, uint32_t k) { return saw_div(b, 0.0007f * (float)(k + 1), 0.01f * (float)k - 0.3f, 1.0f + (float)(k % 5)); }, 1},
        {"min with a row on the left (Sparkle's NaN)", [](Build &b, uint32_t, uint32_t k) {
             return b.op(FR_PRIM_MULTIPLY, Cf(1.0f / (float)(k + 1)), N(b.op(FR_PRIM_MINIMUM, In(0), N(b.op(FR_PRIM_MODULO, In(0), Cf(0.5f + (float)k)))))); }, 1},
    };
    std::mt19937 rng(11);
    uint64_t compared = 0;
    for (const Case &cs : cases)
        for (uint32_t log2_p : {7u, 8u, 10u}) {
            Planned p = planned({{1u << log2_p, cs.leaf}});
            CHECK(p.banks.size() == 1 && p.banks[0].jit && p.banks[0].log2_p == log2_p);
            if (p.banks.size() != 1 || !p.banks[0].jit) continue;
            const BankLaunch &b = p.banks[0];
            LeafProgram lp;
            CHECK(compile_leaf_program(b.shape, b.varying, b.literal_bits, b.alias, lp) && program_well_formed(lp));
            // every leaf's own column values, read back from the bank: a varying column from the table, any other its literal
            const uint32_t P = 1u << log2_p, K = lp.k;
            CHECK(b.params.size() == (size_t)P * K);
            std::vector<std::vector<uint32_t>> consts(P, std::vector<uint32_t>(b.shape.n_consts));
            for (uint32_t i = 0; i < P; ++i) {
                uint32_t j = 0;
                std::vector<uint32_t> col_param(b.shape.n_consts, 0);
                for (uint32_t c = 0; c < b.shape.n_consts; ++c) {
                    if (b.varying[c] && b.alias[c] == c) col_param[c] = j++;
                    consts[i][c] = !b.varying[c] ? b.literal_bits[c] : f32_to_bits(b.params[(size_t)i * K + col_param[b.alias[c]]]);
                }
            }
            for (int sparkle = 0; sparkle < 2; ++sparkle)
                for (uint32_t frame = 0; frame < 40; ++frame) {
                    std::vector<float> rows(8, 0.0f);
                    for (uint32_t r = 0; r < cs.n_in; ++r)
                        rows[r] = frame < 23 ? hostile[(frame + 7 * r) % 23] : std::uniform_real_distribution<float>(-3000.0f, 90000.0f)(rng);
                    std::vector<float> leaves(P);
                    for (uint32_t i = 0; i < P; ++i) leaves[i] = eval_shape(b.shape, consts[i], rows, sparkle != 0);
                    const float expect = sum_rec(leaves, 0, P);
                    for (uint32_t chunk_log2 : {7u, 8u, 10u}) {
                        if (chunk_log2 > log2_p) continue;
                        const float got = model_voice(lp, b.params, log2_p, chunk_log2, rows, sparkle != 0);
                        CHECK(f32_to_bits(got) == f32_to_bits(expect) || (got != got && expect != expect));
                        ++compared;
                    }
                }
        }
    CHECK(compared == 4u * (1 + 2 + 3) * 2 * 40);
}

// ---- the rules --------------------------------------------------------------------------------------------------------------
static void test_serving_rule() {
    {   // the triangle voice: served; each prerequisite missing in turn: today's sentence
        Planned p = planned({{128, tri_leaf()}, {128, tri_leaf()}});
        CHECK(p.banks.size() == 1 && p.banks[0].jit && p.banks[0].rows.size() == 2 && p.sp.progs.empty());
        CHECK(stream_path(p.sp, p.list(), p.env));
        StreamPlan s = p.plan();
        CHECK(s.servable && s.reason.empty() && s.voices == 2 && s.banks.size() == 1 && s.banks[0].leaf && !s.banks[0].general && s.has_leaves() && !s.has_general());
        CHECK(s.leaf_progs.size() == 1 && s.leaf_progs[0].ins.size() == 12 && s.input_slots == std::vector<uint32_t>{0} && s.workgroups() == 2 && s.banks[0].chunk_log2 == 7);
        Planned off = p;
        off.env.leaves = false;
        CHECK(!stream_path(off.sp, off.list(), off.env));
        StreamPlan t = off.plan();
        CHECK(!t.servable && t.reason == OLD_TEMPLATE && t.leaf_progs.empty() && t.banks.empty());
        off.env.general = true;
        CHECK(off.plan().reason == OLD_TEMPLATE_GENERAL);
        Planned noprog = p;                     // FR_STREAM_LEAVES does nothing without FR_STREAM_PROGRAMS
        noprog.env.programs = false;
        CHECK(!stream_path(noprog.sp, noprog.list(), noprog.env) && noprog.plan().reason == OLD_TEMPLATE);
        p.env.device_cus = 256;                 // a whole device: chunks of 128 stay (already the smallest)
        CHECK(p.plan().workgroups() == 2);
    }
    {   // chunks: 512 partials over 4 workgroups each, as a template bank is dealt
        Planned p = planned({{512, tri_leaf()}, {512, tri_leaf()}});
        StreamPlan s = p.plan();
        CHECK(s.servable && s.banks[0].leaf && s.banks[0].chunk_log2 == 7 && s.chunks == 4 && s.workgroups() == 8);
        std::vector<StreamBank> twin(1);
        twin[0].voices = 2; twin[0].log2_p = 9;
        CHECK(deal_stream_chunks(twin, stream_max_wgs(0)) && twin[0].chunk_log2 == s.banks[0].chunk_log2);
    }
    {   // voices of 64 partials; of 32
        for (uint32_t P : {64u, 32u}) {
            Planned p = planned({{P, tri_leaf()}});
            CHECK(p.banks.size() == 1 && p.banks[0].jit);
            StreamPlan s = p.plan();
            CHECK(!s.servable && s.reason == "compiled voices of " + std::to_string(P) +
                                                 " partials; block streaming interprets the leaves of voices of at least 128 partials (16 waves x one group of 8)");
            p.env.general = true;               // (FR_STREAM_GENERAL serves template voices of that size, not these)
            CHECK(p.plan().reason == s.reason);
        }
    }
    {   // a leaf that reads a control row: FR_STREAM_INPUTS, the slot joins input_slots
        Planned p = planned({{128, tri_leaf(1)}});
        CHECK(p.banks.size() == 1 && p.banks[0].jit);
        StreamPlan s = p.plan();
        CHECK(!s.servable && s.reason == "a leaf reads input slot 1; block streaming feeds slot 0 only");
        p.env.inputs = true;
        s = p.plan();
        CHECK(s.servable && s.input_slots == (std::vector<uint32_t>{0, 1}) && s.leaf_progs[0].inputs_read == 2);
        CHECK(stream_launch(p.sp, s).n_rows == 2);
    }
    {   // nine slots in all: the limit of streamed rows counts the leaves' slots
        Planned p = planned({{128, tri_leaf()}});   // (the matcher takes fewer inputs per leaf: the shape is extended by hand)
        p.env.inputs = true;
        CHECK(p.banks.size() == 1 && p.banks[0].jit);
        LeafShape &sh = p.banks[0].shape;
        for (uint32_t slot = 1; slot <= 8; ++slot) {
            sh.input_slots.push_back(slot);
            sh.ops.push_back({OP_INPUT, slot, 0});
            sh.ops.push_back({OP_MUL, (uint32_t)sh.ops.size() - 2u, (uint32_t)sh.ops.size() - 1u});
        }
        CHECK(p.plan().reason == "the leaves and the programs read 9 distinct input slots (slot 0 included); block streaming feeds at most 8");
    }
    {   // a second bank -- a template bank, or a leaf bank of another shape -- needs FR_STREAM_BANKS
        Planned p = planned({{128, tri_leaf()}, {128, [](Build &b, uint32_t, uint32_t k) { return saw_div(b, 0.0007f * (float)(k + 1), 0.01f * (float)k, 2.0f + (float)k); }}});
        CHECK(p.banks.size() == 2 && p.banks[0].jit && p.banks[1].jit);
        CHECK(p.plan().reason == "block streaming needs a plan with one voice bank (this one: 2 bank launches)");
        p.env.banks = true;
        StreamPlan s = p.plan();
        CHECK(s.servable && s.banks.size() == 2 && s.banks[0].leaf && s.banks[1].leaf && s.leaf_progs.size() == 2 && s.leaf_progs[1].ins.size() == 5);
    }
    {   // a track voice
        Planned p = planned({{128, [](Build &b, uint32_t, uint32_t k) {
            const uint32_t x = b.op(FR_PRIM_MULTIPLY, In(0), In(1 + 2 * k));
            return b.op(FR_PRIM_MULTIPLY, In(2 + 2 * k), N(b.op(FR_PRIM_MODULO, N(x), Cf(1.0f)))); }}}, 1);
        CHECK(p.banks.size() == 1 && p.banks[0].jit && p.banks[0].tracks);
        p.env.inputs = true;
        CHECK(p.plan().reason == "these compiled voices read per-leaf track rows (track voices); block streaming interprets leaves over constants and streamed input rows only");
        p.env.leaves = false;
        CHECK(p.plan().reason == OLD_TEMPLATE);
    }
    {   // a chunked compiled bank, a leaf over the limits, a sweep plan: hand-set on the real bank
        Planned p = planned({{128, tri_leaf()}});
        Planned ws = p;
        ws.banks[0].to_ws = true;
        CHECK(ws.plan().reason == "a compiled bank that is cut into chunks over an exchange workspace; block streaming serves whole compiled voices only");
        Planned big = p;
        LeafShape &s = big.banks[0].shape;      // 33 ops: the triangle, then + 0.5 twenty-one times
        while (arith_ops(s) < 33) {
            s.ops.push_back({OP_CONST, 0, 0});
            s.ops.push_back({OP_SUM2, (uint32_t)s.ops.size() - 2u, (uint32_t)s.ops.size() - 1u});
        }
        CHECK(big.plan().reason == "a leaf of 33 arithmetic ops; block streaming interprets leaves of at most 32");
        Planned sweep = p;
        sweep.sp.fused_sweep = 4;
        sweep.env.loops = sweep.env.dyn = sweep.env.sweep = true;
        CHECK(sweep.plan().reason == "a sweep plan (a feedback loop that delays by a signal amount) together with compiled voices; block streaming has no sweep form with a leaf interpreter");
        sweep.env.sweep = false;                // (without FR_STREAM_SWEEP: today's sentence, before any bank is looked at)
        CHECK(sweep.plan().reason == "a feedback loop delays by a signal amount (a sweep plan, FR_LOOP_DYN): block streaming does not serve it");
    }
    {   // a plan without a compiled bank is what it was, with the option on or off (the hand-built plans of the other tests)
        for (StreamKernel k : {StreamKernel::prog, StreamKernel::bus, StreamKernel::in, StreamKernel::banks, StreamKernel::loops, StreamKernel::general, StreamKernel::dyn}) {
            Built b = kernel_plan(k);
            const StreamPlan off = b.plan();
            b.env.leaves = true;
            const StreamPlan on = b.plan();
            CHECK(on.servable && off.servable && on.leaf_progs.empty() && !on.has_leaves() && stream_launch(b.sp, on).kernel == k && stream_launch(b.sp, off).kernel == k);
            CHECK(on.progs == off.progs && on.voice_first == off.voice_first && on.input_slots == off.input_slots && on.workgroups() == off.workgroups());
        }
    }
}

static void test_launch_rule_and_check() {
    CHECK((uint32_t)StreamKernel::leaf == (uint32_t)StreamKernel::sweep_store_fx + 4 && (uint32_t)StreamKernel::leaf_store == (uint32_t)StreamKernel::leaf + 2);
    CHECK(stream_kernel_named(StreamKernel::leaf) && stream_kernel_named(StreamKernel::leaf_store) && !stream_kernel_named((StreamKernel)((uint32_t)StreamKernel::leaf + 1)) &&
          !stream_kernel_named((StreamKernel)((uint32_t)StreamKernel::leaf_store + 1)) && !stream_kernel_named((StreamKernel)((uint32_t)StreamKernel::leaf - 1)));
    CHECK(std::string(stream_kernel_name(StreamKernel::leaf)) == "bank_stream_leaf_kernel" && std::string(stream_kernel_name(StreamKernel::leaf_store)) == "bank_stream_leaf_store_kernel");
    {   // the forms: hist and store, and the flag
        const StreamForm l = stream_form(StreamKernel::leaf), h = stream_form(StreamKernel::hist), ls = stream_form(StreamKernel::leaf_store), st = stream_form(StreamKernel::store);
        CHECK(l.leaf && ls.leaf && !h.leaf && !st.leaf && !l.sweep && !ls.sweep && !l.voiceless && !l.store && ls.store);
        CHECK(l.progs == h.progs && l.bus == h.bus && l.rows == h.rows && l.table == h.table && l.loops == h.loops && l.schedule == h.schedule && l.dyn == h.dyn && l.hist == h.hist);
        CHECK(ls.progs == st.progs && ls.table == st.table && ls.loops == st.loops && ls.schedule == st.schedule && ls.dyn == st.dyn && ls.hist == st.hist);
        for (StreamKernel k : {StreamKernel::plain, StreamKernel::prog, StreamKernel::bus, StreamKernel::in, StreamKernel::banks, StreamKernel::loops, StreamKernel::general,
                               StreamKernel::dyn, StreamKernel::hist, StreamKernel::fx, StreamKernel::store, StreamKernel::store_fx, StreamKernel::sweep, StreamKernel::sweep_fx,
                               StreamKernel::sweep_store, StreamKernel::sweep_store_fx})
            CHECK(!stream_form(k).leaf);
    }
    Planned p = planned({{256, tri_leaf()}, {256, tri_leaf()}});
    p.env.device_cus = 256;
    StreamPlan s = p.plan();
    CHECK(s.servable);
    StreamLaunch l = stream_launch(p.sp, s);
    CHECK(l.kernel == StreamKernel::leaf && l.rows_doorbell && l.own_instrs && l.by_plan && l.bank_table && !l.schedule_table && l.n_rows == 1 && l.hist_cap == 64 &&
          l.workgroups == 4 && l.max_stride == 0);
    Planned st = p;
    st.env.store = true;
    CHECK(stream_launch(st.sp, st.plan()).kernel == StreamKernel::leaf_store && stream_launch(st.sp, st.plan()).hist_cap == 64);

    // the launch check on arguments laid out as the engine lays them out for that plan
    float dummy[4] = {};
    uint32_t words[4] = {};
    uint4 prog_words[12] = {};
    auto args = [&] {
        StreamLaunchArgs x{};
        x.a.leaf_variant = 1; x.a.out = dummy; x.a.n_voices = 2; x.a.ws = dummy; x.a.tickets = words;
        x.ctl_dev = dummy; x.dev = dummy; x.n_rows = 1;
        x.h.hist = dummy; x.h.mask = 63;
        x.p.voice_first = words;
        x.t.n_banks = 1;
        x.t.bank[0] = {(const float2 *)dummy, words, 0, 0, 2, 8, 7, 1, 0};
        x.l.mask = 1;
        x.l.bank[0] = {prog_words, 12, 2, LEAF_REG, 1};
        return x;
    };
    CHECK(stream_launch_check(StreamKernel::leaf, args()) == 4 && stream_launch_check(StreamKernel::leaf_store, args()) == 4);
    CHECK(stream_launch_check(StreamKernel::hist, args()) == 4);                       // (the form underneath does not read the leaf table)
    { StreamLaunchArgs x = args(); x.l.mask = 0; CHECK(stream_launch_check(StreamKernel::leaf, x) == 0); }                 // a leaf form without a leaf bank
    { StreamLaunchArgs x = args(); x.l.mask = 2; CHECK(stream_launch_check(StreamKernel::leaf, x) == 0); }                 // a bank the table does not have
    { StreamLaunchArgs x = args(); x.g.mask = 1; x.g.bank[0] = {words, words}; CHECK(stream_launch_check(StreamKernel::leaf, x) == 0); }   // both a schedule and a leaf bank
    { StreamLaunchArgs x = args(); x.l.bank[0].instrs = nullptr; CHECK(stream_launch_check(StreamKernel::leaf, x) == 0); }
    { StreamLaunchArgs x = args(); x.l.bank[0].n_instr = 33; CHECK(stream_launch_check(StreamKernel::leaf, x) == 0); }
    { StreamLaunchArgs x = args(); x.l.bank[0].k = 0; CHECK(stream_launch_check(StreamKernel::leaf, x) == 0); }
    { StreamLaunchArgs x = args(); x.l.bank[0].result = 8; CHECK(stream_launch_check(StreamKernel::leaf, x) == 0); }
    { StreamLaunchArgs x = args(); x.l.bank[0].result_kind = LEAF_PARAM; x.l.bank[0].result = 2; CHECK(stream_launch_check(StreamKernel::leaf, x) == 0); }
    { StreamLaunchArgs x = args(); x.l.bank[0].result_kind = LEAF_IN; x.l.bank[0].result = 1; CHECK(stream_launch_check(StreamKernel::leaf, x) == 0); }
    { StreamLaunchArgs x = args(); x.l.bank[0] = {nullptr, 0, 1, LEAF_IN, 0}; CHECK(stream_launch_check(StreamKernel::leaf, x) == 4); }   // a bare input: no instructions
    { StreamLaunchArgs x = args(); x.t.bank[0].chunk_log2 = 6; CHECK(stream_launch_check(StreamKernel::leaf, x) == 0); }  // a leaf bank has a template bank's shape
    { StreamLaunchArgs x = args(); x.h.hist = nullptr; CHECK(stream_launch_check(StreamKernel::leaf, x) == 0); }
    CHECK(stream_launch_check((StreamKernel)((uint32_t)StreamKernel::leaf + 1), args()) == 0 && stream_launch_check((StreamKernel)((uint32_t)StreamKernel::sweep_store_fx + 2), args()) == 0);
}

int main() {
    test_compiler();
    test_model();
    test_serving_rule();
    test_launch_rule_and_check();
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
