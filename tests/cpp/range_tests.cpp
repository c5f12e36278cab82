// range_tests.cpp -- CPU tests of the planner's interval arithmetic (csrc/range.hpp) and of what stage.cpp makes of its
// results.  Range::combine decides how far back a ring may be read, what block streaming keeps of an input row, the frames a
// sweep strides by, and (match.cpp) whether a Modulo argument is finite: an interval that is too small for ONE operand pair makes
// a correct kernel give a wrong sample.  Nothing here reads the engine's own evaluation of the primitives: `prim` restates them
// in f32 as the oracle defines them.
//
//   1. one step     every op x {reference, sparkle} x every pair of intervals whose endpoints come from a hostile f32 set
//                   (NaN flag both ways, Range::exactly(c) for every c and NaN): operands inside the intervals -- the four
//                   corners always, the NaN combinations where flagged, and a rotating pick of the other candidates (inward
//                   neighbours of the endpoints, the midpoint, every set member inside) -- must give a result inside the
//                   combined range; a NaN result needs its .nan
//   2. chains       seeded random expressions of depth <= 4 over constants of the set and two inputs in [0, 2^32], evaluated in
//                   f32 at sampled inputs against the composed range (a widening that is too small shows here)
//   3. non-vacuity  at least a quarter of the combined ranges of 1. are finite ("always unbounded" is sound and useless)
//   4. conversions  lower + plan_stages: amounts whose proven top is just below, at and above 2^31; a negative top (0 frames);
//                   a NaN constant amount; Planner::dyn_lo for lower bounds 0.5, 1.0, 1.5, 2^31 and a may-be-NaN amount
//
// Build: g++ -std=c++17 -O2 -ffp-contract=off -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -o range_tests range_tests.cpp -ldl
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>

#include "../../libfriendship_amd/csrc/graph.cpp"
#include "../../libfriendship_amd/csrc/match.cpp"
#include "../../libfriendship_amd/csrc/stage.cpp"
#include "../../libfriendship_amd/csrc/stagejit.cpp"
#include "../../libfriendship_amd/csrc/leafjit.cpp"

using namespace fr;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); throw std::runtime_error("check failed"); } } while (0)

static const uint32_t OPS[5] = {OP_SUM2, OP_MUL, OP_DIV, OP_MOD, OP_MIN};
static const char *op_name(uint32_t op) { return op == OP_SUM2 ? "Sum2" : op == OP_MUL ? "Multiply" : op == OP_DIV ? "Divide" : op == OP_MOD ? "Modulo" : "Minimum"; }

// the primitives in f32, as the oracle defines them (this file is built with -ffp-contract=off)
static float prim(uint32_t op, float a, float b, bool sparkle) {
    switch (op) {
    case OP_SUM2: return a + b;
    case OP_MUL: return a * b;
    case OP_DIV: return a / b;
    case OP_MOD: { float r = fmodf(a, b); return r < 0.0f ? r + b : r; }
    default:
        if (sparkle && a != a) return a;
        return (a < b || b != b) ? a : b;
    }
}

static const float TWO24 = 16777216.0f, TWO32 = 4294967296.0f, TWO63 = 9223372036854775808.0f, TWO64 = 18446744073709551616.0f;
static std::vector<float> hostile_set() {
    const float ulp_up = std::nextafterf(1.0f, 2.0f), ulp_dn = std::nextafterf(1.0f, 0.0f);
    // (2^24 + 1 is not an f32: its neighbour 2^24 + 2 stands for "the first integer the format skips")
    std::vector<float> s = {0.0f, -0.0f, 1e-45f, -1e-45f, FLT_MIN, -FLT_MIN, 1e-30f, -1e-30f, 0.5f, -0.5f, 0.75f, -0.75f, 1.0f, -1.0f, ulp_up, ulp_dn,
                            1.5f, 3.0f, -3.0f, 7.0f, -7.0f, 48000.0f, -48000.0f, TWO24, TWO24 + 2.0f, TWO32, -TWO32, TWO63, TWO64, 1e30f, -1e30f,
                            3e38f, -3e38f, FLT_MAX, -FLT_MAX, HUGE_VALF, -HUGE_VALF};
    std::sort(s.begin(), s.end(), [](float a, float b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); });
    return s;
}

struct Interval {
    Range r;
    std::vector<float> members;   // operands inside: the corners first (lo, hi), then the other candidates
    bool nan;
};

static std::vector<Interval> intervals(const std::vector<float> &S) {
    std::vector<Interval> out;
    for (size_t i = 0; i < S.size(); ++i)
        for (size_t j = i; j < S.size(); ++j)
            for (int nan = 0; nan < 2; ++nan) {
                const float lo = S[i], hi = S[j];
                Interval iv;
                iv.r = i == j ? Range::exactly(lo) : Range{(double)lo, (double)hi, false};
                iv.r.nan = nan != 0;
                iv.nan = nan != 0;
                iv.members = {lo, hi};
                if (i != j) {
                    const float up = std::nextafterf(lo, HUGE_VALF), dn = std::nextafterf(hi, -HUGE_VALF);
                    if (up <= hi) iv.members.push_back(up);
                    if (dn >= lo) iv.members.push_back(dn);
                    if (std::isfinite(lo) && std::isfinite(hi)) iv.members.push_back((float)(((double)lo + (double)hi) * 0.5));
                    for (size_t k = i + 1; k < j; ++k) iv.members.push_back(S[k]);
                }
                for (float m : iv.members) CHECK((double)m >= iv.r.lo && (double)m <= iv.r.hi);
                out.push_back(iv);
            }
    Interval n;   // Range::exactly(NaN): no value but NaN
    n.r = Range::exactly(std::nanf(""));
    n.nan = true;
    CHECK(n.r.nan);
    out.push_back(n);
    return out;
}

static uint64_t g_checks = 0, g_ranges = 0, g_finite = 0, g_failures = 0;

static void check_one(uint32_t op, bool sparkle, const Range &A, const Range &B, const Range &R, float a, float b) {
    ++g_checks;
    const float r = prim(op, a, b, sparkle);
    const bool ok = r != r ? R.nan : ((double)r >= R.lo && (double)r <= R.hi);
    if (ok) return;
    if (++g_failures <= 20)
        std::fprintf(stderr, "UNSOUND %s%s: a = %.9g in [%.17g, %.17g]%s, b = %.9g in [%.17g, %.17g]%s: result %.9g outside [%.17g, %.17g]%s\n", op_name(op),
                     sparkle ? " (sparkle)" : "", a, A.lo, A.hi, A.nan ? " or NaN" : "", b, B.lo, B.hi, B.nan ? " or NaN" : "", r, R.lo, R.hi, R.nan ? " or NaN" : "");
}

static bool same_range(const Range &x, const Range &y) { return std::memcmp(&x.lo, &y.lo, sizeof(double)) == 0 && std::memcmp(&x.hi, &y.hi, sizeof(double)) == 0 && x.nan == y.nan; }

static void one_step() {
    const std::vector<float> S = hostile_set();
    const std::vector<Interval> I = intervals(S);
    const float qnan = std::nanf("");
    uint64_t rot = 0;
    for (uint32_t op : OPS)
        for (int sparkle = 0; sparkle < 2; ++sparkle)
            for (const Interval &A : I)
                for (const Interval &B : I) {
                    const Range R = Range::combine(op, A.r, B.r, sparkle != 0);
                    if (op != OP_MIN && sparkle) {   // the semantics part at Minimum only: the same range, checked once
                        if (!same_range(R, Range::combine(op, A.r, B.r, false))) { ++g_failures; std::fprintf(stderr, "%s: the range depends on the semantics\n", op_name(op)); }
                        continue;
                    }
                    ++g_ranges;
                    g_finite += R.finite() ? 1 : 0;
                    const size_t na = A.members.size(), nb = B.members.size();
                    for (size_t i = 0; i < std::min<size_t>(na, 2); ++i)
                        for (size_t j = 0; j < std::min<size_t>(nb, 2); ++j) check_one(op, sparkle, A.r, B.r, R, A.members[i], B.members[j]);
                    if (A.nan) for (size_t j = 0; j < std::min<size_t>(nb, 2); ++j) check_one(op, sparkle, A.r, B.r, R, qnan, B.members[j]);
                    if (B.nan) for (size_t i = 0; i < std::min<size_t>(na, 2); ++i) check_one(op, sparkle, A.r, B.r, R, A.members[i], qnan);
                    if (A.nan && B.nan) check_one(op, sparkle, A.r, B.r, R, qnan, qnan);
                    // the other candidates, thinned: a pick that rotates through the cross product from one interval pair to the
                    // next (Modulo is not monotone: its extremes are not at the corners, so it gets more picks)
                    if (na * nb > 4) {
                        const int picks = op == OP_MOD ? 4 : 2;
                        for (int k = 0; k < picks; ++k) {
                            rot += 0x9E3779B97F4A7C15ull;
                            const uint64_t q = (rot >> 17) % (na * nb);
                            check_one(op, sparkle, A.r, B.r, R, A.members[q / nb], B.members[q % nb]);
                        }
                    }
                }
    std::printf("one step: %llu intervals, %llu ranges (%llu finite), %llu checks\n", (unsigned long long)I.size(), (unsigned long long)g_ranges,
                (unsigned long long)g_finite, (unsigned long long)g_checks);
    CHECK(g_failures == 0);
    CHECK(g_checks >= 50000000ull);
    CHECK(4 * g_finite >= g_ranges);   // non-vacuity
}

// ---- chains ---------------------------------------------------------------------------------------------------------
struct Expr { int kind; uint32_t op; float c; int a, b; };   // kind 0: constant, 1: input x, 2: input y, 3: op(a, b)

static int random_expr(std::vector<Expr> &e, std::mt19937 &rng, const std::vector<float> &S, int depth) {
    const uint32_t leaf = rng() % 8;
    if (depth == 0 || leaf < 2) {
        const uint32_t k = rng() % 3;
        if (k == 0) e.push_back({0, 0, S[rng() % S.size()], -1, -1});
        else e.push_back({(int)k, 0, 0.0f, -1, -1});
        return (int)e.size() - 1;
    }
    const uint32_t op = OPS[rng() % 5];
    const int a = random_expr(e, rng, S, depth - 1), b = random_expr(e, rng, S, depth - 1);
    e.push_back({3, op, 0.0f, a, b});
    return (int)e.size() - 1;
}

static void chains() {
    std::vector<float> S = hostile_set();
    S.push_back(std::nanf(""));
    std::mt19937 rng(0x5EED0A01u);
    std::vector<float> xs = {0.0f, TWO32, 1e-45f, 0.5f, 1.0f, 2.0f, 8388608.5f, TWO24, 48000.0f, std::nextafterf(TWO32, 0.0f), 0.999999940f, 3.0f};
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    for (int i = 0; i < 12; ++i) xs.push_back(std::ldexp(u(rng), (int)(rng() % 33)));   // random magnitudes up to 2^32
    for (float x : xs) CHECK(x >= 0.0f && x <= TWO32);
    uint64_t exprs = 0, finite = 0, checks = 0, failures = 0;
    for (int n = 0; n < 20000; ++n) {
        std::vector<Expr> e;
        const int root = random_expr(e, rng, S, 1 + (int)(rng() % 4));
        for (int sparkle = 0; sparkle < 2; ++sparkle) {
            std::vector<Range> r(e.size());
            for (size_t i = 0; i < e.size(); ++i)
                r[i] = e[i].kind == 0 ? Range::exactly(e[i].c) : e[i].kind != 3 ? Range{0.0, 4294967296.0, false} : Range::combine(e[i].op, r[e[i].a], r[e[i].b], sparkle != 0);
            ++exprs;
            finite += r[root].finite() ? 1 : 0;
            std::vector<float> v(e.size());
            for (float x : xs)
                for (float y : xs) {
                    for (size_t i = 0; i < e.size(); ++i)
                        v[i] = e[i].kind == 0 ? e[i].c : e[i].kind == 1 ? x : e[i].kind == 2 ? y : prim(e[i].op, v[e[i].a], v[e[i].b], sparkle != 0);
                    for (size_t i = 0; i < e.size(); ++i) {   // every sub-expression against its composed range
                        ++checks;
                        const bool ok = v[i] != v[i] ? r[i].nan : ((double)v[i] >= r[i].lo && (double)v[i] <= r[i].hi);
                        if (!ok && ++failures <= 10)
                            std::fprintf(stderr, "UNSOUND chain %d%s node %zu (%s): x = %.9g, y = %.9g: %.9g outside [%.17g, %.17g]%s\n", n, sparkle ? " (sparkle)" : "", i,
                                         e[i].kind == 3 ? op_name(e[i].op) : "leaf", x, y, v[i], r[i].lo, r[i].hi, r[i].nan ? " or NaN" : "");
                    }
                }
        }
    }
    std::printf("chains: %llu expressions (%llu with a finite range), %llu checks\n", (unsigned long long)exprs, (unsigned long long)finite, (unsigned long long)checks);
    CHECK(failures == 0);
    CHECK(4 * finite >= exprs);
}

// ---- conversions: what stage.cpp makes of a range ----------------------------------------------------------------------
struct Operand { int kind; uint32_t v; };   // 0 = node handle, 1 = constant bits, 2 = input slot
static Operand N(uint32_t h) { return {0, h}; }
static Operand Cf(float f) { return {1, f32_to_bits(f)}; }
static Operand In(uint32_t s) { return {2, s}; }

struct Build {
    std::vector<std::pair<uint32_t, int>> nodes{{1, FR_PRIM_F32CONSTANT}};
    std::vector<fr_edge> edges;
    uint32_t next = 2;
    void connect(Operand o, uint32_t to, uint32_t slot) {
        if (o.kind == 0) edges.push_back({o.v, to, 0, slot});
        else if (o.kind == 1) edges.push_back({1, to, o.v, slot});
        else edges.push_back({0, to, o.v, slot});
    }
    uint32_t node(int kind) { nodes.push_back({next, kind}); return next++; }
    uint32_t op(int kind, Operand a, Operand b) {
        const uint32_t h = node(kind);
        connect(a, h, 0);
        connect(b, h, 1);
        return h;
    }
    FlatGraph lowered(uint32_t n_slots) const {
        Mirror m;
        for (auto &n : nodes) { fr_effect e{}; e.kind = n.second; m.add_node(n.first, &e); }
        for (auto &e : edges) m.add_edge(e);
        return lower(m, n_slots);
    }
};

// Delay(source, Minimum(C(top), In1)): Minimum's upper bound is the constant itself (it is not widened)
static Build capped_delay(float top, bool of_input) {
    Build b;
    const uint32_t amt = b.op(FR_PRIM_MINIMUM, Cf(top), In(1));
    const uint32_t d = of_input ? b.op(FR_PRIM_DELAY, In(0), N(amt)) : b.op(FR_PRIM_DELAY, N(b.op(FR_PRIM_MULTIPLY, In(0), Cf(0.5f))), N(amt));
    b.connect(N(d), 0, 0);
    return b;
}

static const StageInstr *find_instr(const StagedPlan &sp, uint32_t op) {
    for (const StageInstr &in : sp.instrs) if (in.op == op) return &in;
    return nullptr;
}

static void conversions() {
    const float below = std::nextafterf(2147483648.0f, 0.0f), at = 2147483648.0f, above = std::nextafterf(2147483648.0f, HUGE_VALF);
    CHECK(below == 2147483520.0f);
    // a ring's look-back: staged only while the proven top converts to frames below 2^31, and then it covers the top
    for (float top : {48.0f, below, at, above}) {
        FlatGraph fg = capped_delay(top, false).lowered(1);
        StagedPlan sp = plan_stages(fg, false, true, 20);
        if (top < at) {
            CHECK(sp.pull_rows.empty() && find_instr(sp, S_READ_DYN));
            CHECK(sp.lmax == (uint64_t)top);
        } else {
            CHECK(sp.pull_rows.size() == 1 && sp.lmax == 0);
        }
    }
    // an input delayed by a signal needs no ring; block streaming reads the bound from S_READ_INPUT_DYN's buf (none: 0xFFFFFFFF)
    for (float top : {48.0f, below, at, above, -3.0f}) {
        FlatGraph fg = capped_delay(top, true).lowered(1);
        StagedPlan sp = plan_stages(fg, false, true, 20);
        const StageInstr *in = find_instr(sp, S_READ_INPUT_DYN);
        CHECK(sp.pull_rows.empty() && in);
        CHECK(in->buf == (top < 0.0f ? 0u : top < at ? (uint32_t)top : 0xFFFFFFFFu));
    }
    {   // a negative top: 0 frames
        FlatGraph fg = capped_delay(-3.0f, false).lowered(1);
        StagedPlan sp = plan_stages(fg, false, true, 20);
        CHECK(sp.pull_rows.empty() && sp.lmax == 0);
    }
    {   // a NaN constant amount delays by 0 frames: no look-back, no signal read
        Build b;
        const uint32_t d = b.op(FR_PRIM_DELAY, N(b.op(FR_PRIM_MULTIPLY, In(0), Cf(0.5f))), Cf(std::nanf("")));
        b.connect(N(d), 0, 0);
        FlatGraph fg = b.lowered(1);
        StagedPlan sp = plan_stages(fg, false, true, 20);
        CHECK(sp.pull_rows.empty() && sp.lmax == 0 && !find_instr(sp, S_READ_DYN));
    }
    // Planner::dyn_lo: the frames a sweep may stride by.  guard = Minimum(C(4), Modulo(In1, 4)) is in [0, 4] and never NaN;
    // Sum2 widens outward (a whole `lo` loses a frame), Minimum keeps the smaller lower bound as it is.
    struct DynLo { const char *what; std::function<uint32_t(Build &)> amount; double least; uint64_t expect; };
    auto guard = [](Build &b) { return b.op(FR_PRIM_MINIMUM, Cf(4.0f), N(b.op(FR_PRIM_MODULO, In(1), Cf(4.0f)))); };
    const std::vector<DynLo> cases = {
        {"0.5 + guard", [&](Build &b) { return b.op(FR_PRIM_SUM2, Cf(0.5f), N(guard(b))); }, 0.5, 0},
        {"1.0 + guard", [&](Build &b) { return b.op(FR_PRIM_SUM2, Cf(1.0f), N(guard(b))); }, 1.0, 0},
        {"1.5 + guard", [&](Build &b) { return b.op(FR_PRIM_SUM2, Cf(1.5f), N(guard(b))); }, 1.5, 1},
        {"3.0 + guard", [&](Build &b) { return b.op(FR_PRIM_SUM2, Cf(3.0f), N(guard(b))); }, 3.0, 2},
        {"Minimum(1.0, 2 + guard)", [&](Build &b) { return b.op(FR_PRIM_MINIMUM, Cf(1.0f), N(b.op(FR_PRIM_SUM2, Cf(2.0f), N(guard(b))))); }, 1.0, 1},
        {"Minimum(2^31, 2^32 + guard)", [&](Build &b) { return b.op(FR_PRIM_MINIMUM, Cf(2147483648.0f), N(b.op(FR_PRIM_SUM2, Cf(4294967296.0f), N(guard(b))))); }, 2147483648.0, 0x7FFFFFFFull},
        {"3 + Modulo(In1, 4): NaN for In1 = inf", [&](Build &b) { return b.op(FR_PRIM_SUM2, Cf(3.0f), N(b.op(FR_PRIM_MODULO, In(1), Cf(4.0f)))); }, 0.0, 0},
    };
    for (const DynLo &c : cases) {
        Build b;
        const uint32_t d = b.op(FR_PRIM_DELAY, N(b.op(FR_PRIM_MULTIPLY, In(0), Cf(0.5f))), N(c.amount(b)));
        b.connect(N(d), 0, 0);
        FlatGraph fg = b.lowered(1);
        uint32_t delay = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < fg.nodes.size(); ++i)
            if (fg.nodes[i].op == OP_DELAY && !fg.is_const(fg.nodes[i].b)) delay = i;
        CHECK(delay != 0xFFFFFFFFu);
        Planner P(fg, nullptr);
        CHECK(P.dyn_lo(delay) == 0);                 // (nothing asked for the amount's range yet)
        const Range r = P.range(fg.nodes[delay].b);
        const uint64_t lo = P.dyn_lo(delay);
        if (lo != c.expect) std::fprintf(stderr, "dyn_lo(%s) = %llu, expected %llu (range [%.17g, %.17g]%s)\n", c.what, (unsigned long long)lo, (unsigned long long)c.expect, r.lo, r.hi, r.nan ? " or NaN" : "");
        CHECK(lo == c.expect);
        CHECK((double)lo <= std::floor(c.least));   // soundness: never more frames than the least amount
    }
    std::printf("conversions ok\n");
}

int main() {
    int passed = 0, failed = 0;
    struct T { const char *name; void (*fn)(); } tests[] = {{"one_step", one_step}, {"chains", chains}, {"conversions", conversions}};
    for (const T &t : tests) {
        try { t.fn(); ++passed; std::printf("ok   %s\n", t.name); }
        catch (const std::exception &ex) { ++failed; std::printf("FAIL %s: %s\n", t.name, ex.what()); }
    }
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
