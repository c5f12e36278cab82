// Dense forward f32 reference for graphs with feedback through Delays of a signal amount (TEST INFRASTRUCTURE; the loop that
// tests/loop_dyn_reference.py prepares and calls).  Every node is evaluated ONCE per frame, frames in time order, nodes within a
// frame in the order the caller gives -- a topological order of the graph without the source edges of the Delays that close a
// loop.  The operation rules are tests/stage_reference.py's (reference.rs:178-265):
//     Sum2 / Multiply / Divide   one IEEE f32 operation
//     Modulo                     fmodf, then + b when the result is negative
//     Minimum                    (a < b || b != b) ? a : b; sparkle: a NaN left operand wins
//     Delay                      amount -> frames: NaN or negative -> 0, >= 2^64 -> the output is 0, else floor; sparkle: an amount
//                                that is not >= 0 makes the output 0; before time 0 the value is 0
//     input reads                beyond what the row holds -> 0
// A Delay that closes a loop (flag `loop`) must reach at least one frame back at every frame: a frame where it does not is the
// error the function returns (-(frame + 1)) -- the reference never reads a value it has not computed.  So must a Delay whose
// source comes later in the order (there is none in a correct order).  Built without -ffast-math and without contraction.
#include <cmath>
#include <cstdint>
#include <cstring>

namespace {
enum Kind : int32_t { SUM2 = 0, MUL = 1, DIV = 2, MOD = 3, MIN = 4, DELAY = 5 };
enum Src : int32_t { NONE = 0, CONST = 1, INPUT = 2, NODE = 3 };
struct Operand { int32_t src; uint32_t arg; };   // CONST: f32 bits; INPUT: slot; NODE: index
struct Node { int32_t kind; int32_t loop; Operand a, b; };
}  // namespace

extern "C" int64_t loopdyn_render(const Node *nodes, int32_t n_nodes, const int32_t *order, const float *const *inputs, const int64_t *input_len,
                                  int32_t n_inputs, int64_t end, int32_t sparkle, float *val /* [n_nodes][end] */) {
    auto at = [&](const Operand &o, int64_t t) -> float {
        switch (o.src) {
        case CONST: { float v; std::memcpy(&v, &o.arg, 4); return v; }
        case INPUT: return (int32_t)o.arg < n_inputs && t < input_len[o.arg] ? inputs[o.arg][t] : 0.0f;
        case NODE: return val[(int64_t)o.arg * end + t];
        default: return 0.0f;
        }
    };
    // position of every node in the order: a read 0 frames back needs its source evaluated already
    int32_t *pos = new int32_t[n_nodes];
    for (int32_t i = 0; i < n_nodes; ++i) pos[order[i]] = i;
    int64_t err = 0;
    for (int64_t t = 0; t < end && !err; ++t)
        for (int32_t i = 0; i < n_nodes; ++i) {
            const int32_t h = order[i];
            const Node &n = nodes[h];
            float v;
            if (n.kind == DELAY) {
                const float d = at(n.b, t);
                v = 0.0f;
                bool live = !(d >= 18446744073709551616.0f);
                if (sparkle && !(d >= 0.0f)) live = false;
                if (live) {
                    const double dd = d >= 0.0f ? std::floor((double)d) : 0.0;   // NaN or negative: 0 frames
                    if (dd <= (double)t) {
                        const int64_t fr = (int64_t)dd;
                        if (fr == 0 && n.a.src == NODE && (n.loop || pos[n.a.arg] > i)) { err = -(t + 1); break; }
                        v = at(n.a, t - fr);
                    }
                }
            } else {
                const float a = at(n.a, t), b = at(n.b, t);
                switch (n.kind) {
                case SUM2: v = a + b; break;
                case MUL: v = a * b; break;
                case DIV: v = a / b; break;
                case MOD: { const float r = std::fmod(a, b); v = r < 0.0f ? r + b : r; break; }
                default: v = (a < b || b != b) ? a : b; if (sparkle && a != a) v = a; break;
                }
            }
            val[(int64_t)h * end + t] = v;
        }
    delete[] pos;
    return err;
}
