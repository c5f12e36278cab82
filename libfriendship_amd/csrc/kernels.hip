// kernels.hip -- gfx950 (CDNA4) kernels of the render engine.  Written for 64-lane wavefronts,
// 256 CUs x 4 SIMD-32; compiled with -ffp-contract=off: every f32 operation of the reference
// evaluator (reference src/render/reference.rs:197-262) rounds exactly once and so must we.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "kernels.hpp"

#pragma clang fp contract(off)

namespace fr {

// Diagnostic build only (tools/fewvoice_diag.hip defines FR_DIAG_STAMPS): per-wave timestamps (s_memrealtime at 100 MHz,
// s_memtime on the shader clock) and placement (HW_ID, XCC_ID), written to a buffer the tool hangs on g_diag.  In the
// product no stamp executes and none of this exists.
#ifdef FR_DIAG_STAMPS
__device__ unsigned long long *g_diag = nullptr;     // [workgroup][16 waves][8]: start, compute done, end, HW_ID | XCC_ID << 32, then the
                                                     // same three moments on the shader clock in slots 4..6
#define FR_DIAG_MARK(slot)                                                                                                 \
    do {                                                                                                                   \
        if (g_diag && (threadIdx.x & 63u) == 0u) {                                                                         \
            unsigned long long v_ = __builtin_amdgcn_s_memrealtime();                                                      \
            if ((slot) == 3) v_ = (unsigned long long)__builtin_amdgcn_s_getreg(0xF804) | ((unsigned long long)(__builtin_amdgcn_s_getreg(0xF814) & 15u) << 32); \
            g_diag[((size_t)blockIdx.x * 16u + (threadIdx.x >> 6)) * 8u + (slot)] = v_;                                    \
            if ((slot) != 3) g_diag[((size_t)blockIdx.x * 16u + (threadIdx.x >> 6)) * 8u + 4u + (slot)] = __builtin_amdgcn_s_memtime(); \
        }                                                                                                                  \
    } while (0)
#else
#define FR_DIAG_MARK(slot) do { } while (0)
#endif

// ---------------------------------------------------------------------------------------------------
// Shared primitive arithmetic (bit-exact restatement of reference.rs:197-262)
// ---------------------------------------------------------------------------------------------------
enum : uint32_t { OP_CONST = 0, OP_INPUT = 1, OP_DELAY = 2, OP_SUM2 = 3, OP_MUL = 4, OP_DIV = 5, OP_MOD = 6, OP_MIN = 7 };

__device__ __forceinline__ float prim_mod(float a, float b) {
    // `dividend % divisor` is fmodf (exact, sign of the dividend); `if rem < 0 { rem + divisor }`
    float rem = fmodf(a, b);
    return rem < 0.0f ? rem + b : rem;
}

__device__ __forceinline__ float prim_min(float a, float b, bool sparkle = false) {
    // RefRenderer: Rust >= 1.20 core f32::min: (a < b || b.is_nan()) ? a : b.
    // SparkleRenderer (sparkle.rs:495-496): select(fcmp ult a, b, a, b) -- differs only for a NaN `a` beside a number.
    // The value selected for `b` passes through an empty asm: where the compiler can prove an operand is not NaN (a literal,
    // or a 0.0 it has threaded in from an out-of-range read) the AMDGPU backend rewrites `x < c ? x : c` as v_min_f32, which
    // answers -0 for the tie (-0, +0) where this rule answers `b` (found by tools/stress_parity.py in generated code with a
    // literal zero operand; profiles/r02_stress_parity.txt).  Arms that are not the compare's operands cannot be matched.
    if (sparkle && a != a) return a;
    const bool take_a = a < b || b != b;
    float other = b;
    asm("" : "+v"(other));
    return take_a ? a : other;
}

// dst = a op b: THE arithmetic step of every evaluator here.  pull_kernel passes a node's OP_*, the five stage interpreters
// (stage_kernel, stage_tile_kernel, stage_sweep_kernel, stream_run_programs, stream_run_loop_program) an instruction's S_*
// through STAGE_ARITH_CASES.
__device__ __forceinline__ float prim_binop(uint32_t op, float a, float b, bool sparkle = false) {
    switch (op) {
    case OP_SUM2: return a + b;
    case OP_MUL: return a * b;
    case OP_DIV: return a / b;   // hipcc default: correctly rounded f32 divide
    case OP_MOD: return prim_mod(a, b);
    default: return prim_min(a, b, sparkle);
    }
}
// The arithmetic cases of an interpreter's instruction switch, `v = x op y; break;` each: the S_* -> OP_* mapping, written once.
// Cases of the interpreter's OWN switch, each op a constant, and not one case that hands in.op to prim_binop: that would be a
// second dispatch per instruction, which the interpreters' time shows (profiles/stage_step.txt); this way every interpreter
// compiles to the instructions it has with the cases spelled out.
#define STAGE_ARITH_CASES(v, x, y, sparkle)                     \
    case S_SUM2: v = prim_binop(OP_SUM2, x, y, sparkle); break; \
    case S_MUL: v = prim_binop(OP_MUL, x, y, sparkle); break;   \
    case S_DIV: v = prim_binop(OP_DIV, x, y, sparkle); break;   \
    case S_MOD: v = prim_binop(OP_MOD, x, y, sparkle); break;   \
    case S_MIN: v = prim_binop(OP_MIN, x, y, sparkle); break;

// Delay's amount -> frames (reference.rs:200-211).  Returns false when the output is 0: the amount is >= 2^64, or --
// SparkleRenderer only, sparkle.rs:531-534 -- it is negative or NaN (`ult 0`), where RefRenderer delays by 0 frames.
__device__ __forceinline__ bool delay_frames(float d, uint64_t &frames, bool sparkle = false) {
    if (d >= 18446744073709551616.0f) return false;
    if (sparkle && !(d >= 0.0f)) return false;
    frames = (d < 0.0f || d != d) ? 0ull : (uint64_t)d;   // clamp negatives, NaN -> 0, floor
    return true;
}

__device__ __forceinline__ float read_input(const DevInput *in, uint32_t n_in, uint32_t slot, uint64_t t) {
    if (slot >= n_in) return 0.0f;
    DevInput s = in[slot];
    if (t < s.base || t >= s.len) return 0.0f;   // zero prefix after a seek; beyond stored -> 0 (reference.rs:92-94)
    return s.data[t - s.base];
}

// ---------------------------------------------------------------------------------------------------
// Pull interpreter: one thread per (output row, t), the reference's recursion with an explicit stack.
// Universal (any DAG of the 7 primitives, signal-dependent delays) and bit-exact; cost grows with the
// number of root-to-leaf paths exactly like the reference, so the planner uses it only for graphs
// it cannot stage.  Stack frames live in global memory, [level][thread] so a wave's accesses coalesce.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) pull_kernel(PullArgs a) {
    uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.count) return;
    const uint64_t lin = a.first + e;
    const uint32_t slot = (uint32_t)(lin / a.n_times);
    const uint64_t ti = lin - (uint64_t)slot * a.n_times;

    uint32_t sp = 0;
    uint32_t cur = a.outputs[slot];
    uint64_t cur_t = a.idx + ti;
    float ret = 0.0f;
    bool calling = true;
    for (;;) {
        if (calling) {
            DevNode n = a.nodes[cur];
            if (n.op == OP_CONST) {
                ret = __uint_as_float(n.a);
                calling = false;
            } else if (n.op == OP_INPUT) {
                ret = read_input(a.inputs, a.n_inputs, n.a, cur_t);
                calling = false;
            } else {
                // frame {node, stage 0, t}; first operand: Delay evaluates its amount first (reference.rs:200)
                uint64_t o = (uint64_t)sp * a.count + e;
                a.st_node[o] = cur;
                a.st_time[o] = cur_t;
                ++sp;
                cur = (n.op == OP_DELAY) ? n.b : n.a;
            }
        } else {
            if (sp == 0) break;
            uint64_t o = (uint64_t)(sp - 1) * a.count + e;
            uint32_t ns = a.st_node[o];
            uint32_t node = ns & 0x3FFFFFFFu;
            DevNode n = a.nodes[node];
            uint64_t t = a.st_time[o];
            if ((ns >> 30) == 0) {
                if (n.op == OP_DELAY) {
                    uint64_t frames;
                    --sp;   // tail call: the source's value is the Delay's value
                    if (!delay_frames(ret, frames, a.sparkle != 0u) || frames > t) {
                        ret = 0.0f;   // >= 2^64 or t - frames underflows (reference.rs:202-205,213)
                    } else {
                        cur = n.a;
                        cur_t = t - frames;
                        calling = true;
                    }
                } else {
                    a.st_val[o] = ret;
                    a.st_node[o] = node | (1u << 30);
                    cur = n.b;
                    cur_t = t;
                    calling = true;
                }
            } else {
                ret = prim_binop(n.op, a.st_val[o], ret, a.sparkle != 0u);
                --sp;
            }
        }
    }
    a.out[lin] = ret;
}

hipError_t launch_pull(const PullArgs &a, hipStream_t s) {
    if (a.count == 0) return hipSuccess;
    uint64_t blocks = (a.count + 255) / 256;
    hipLaunchKernelGGL(pull_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Fused oscillator bank.
//
// For each voice v (an output row) and frame t:
//     out[v][t] = TREE_{k<P}  amp_k * parab(Modulo(time[t] * w_k, 1))
// where TREE is the balanced binary Sum2 tree over consecutive leaves and parab is the parabolic sine
//     u = phase + (-0.5);  y = (-16*u) * (0.5 + -(-(min(u, -u))))          (11 primitive nodes per partial)
// Algebra that is exact in f32 (proved in DESIGN.md, checked bit-for-bit by tests/test_bank_parity.py):
//     -(-min(u,-u)) == |u| up to the sign of zero, which 0.5 + (-x) discards;
//     (-16*u)*q == -16*RN(u*q) because |u*q| is 0 or >= 2^-50 (no subnormal, no overflow);
//     amp*(-16*z) == RN((-16*amp)*z) when -16*amp is exact (host checks) -> A = -16*amp.
// So a leaf costs 6 VALU ops (mul, fract, sub, sub|abs|, mul, mul) -- and 5 with two FMAs, see bank_leaf --
// and the tree 1 add: 6 VALU ops per partial-frame on the common path.
//
// Mapping (time-major lanes): a lane owns F frames, a wave owns 64*F consecutive frames and a
// contiguous quarter of the voice's partials, a 256-thread workgroup (4 waves) owns one
// (voice, time-tile).  Partial parameters {w, A} are wave-uniform, so they arrive through the scalar
// cache into SGPRs (s_load_dwordx16 = 8 partials) and feed the VALU as scalar operands: no LDS
// traffic, no cross-lane reduction in the hot loop.  The Sum2 tree is evaluated in its own
// association: 8 leaves in registers, then a binary-counter carry chain of named registers across
// groups (wave-uniform branches), then the 4 waves' subtrees combine through LDS.
// ---------------------------------------------------------------------------------------------------

// EXACT = false is the 5-op leaf: with u2 = 2u = RN(2r - 1) (scaling by 2 commutes with rounding) and
// q = 0.5 - |u| always exact (r is a multiple of 2^-25 wherever |u| < 0.25, Sterbenz elsewhere),
//     u*q = RN(u*(0.5 - |u|)) = (1/4) * RN(u2 - u2*|u2|) = (1/4) * fma(-|u2|, u2, u2)
// so leaf = A4 * fma(-|u2|, u2, u2) with A4 = -4*amp: mul, fract, fma, fma, mul.  It differs from the
// graph's value only in the SIGN OF A ZERO leaf (r = 0: the fma's exact cancellation is +0, the
// graph's product u*(+0) is -0).  A zero's sign cannot change a non-zero sum, so a wave's subtree sum
// is exact whenever it is non-zero; when it is zero the wave recomputes its subtree with EXACT = true,
// the 6-op product form, which is bit-identical to the graph including zero signs
// (both claims brute-forced over 1.5e8 (t, w, amp) triples; parity-tested on device).
template <bool FAST, bool EXACT>
__device__ __forceinline__ float bank_leaf(float t, float w, float A4) {
    float x = t * w;
    float r;
    if (FAST) {
        r = __builtin_amdgcn_fractf(x);   // x >= 0 finite: x - floor(x) == fmodf(x, 1) exactly
    } else {
        r = x - truncf(x);                // == fmodf(x, 1) for every finite x; inf -> NaN like fmodf
        r = r < 0.0f ? r + 1.0f : r;      // `if rem < 0 { rem + divisor }`
    }
    if (EXACT) {
        float u = r - 0.5f;
        float q = 0.5f - fabsf(u);
        float z = u * q;
        return (4.0f * A4) * z;           // -16*amp, exact scaling
    }
    float u2 = __builtin_fmaf(r, 2.0f, -1.0f);
    float z4 = __builtin_fmaf(-fabsf(u2), u2, u2);
    return A4 * z4;
}

typedef float __attribute__((address_space(4))) const *const_f32_ptr;   // constant addrspace -> SMEM loads

struct ParamGroup {   // 8 partials' {w, A}: one s_load_dwordx16, lives in SGPRs
    float w[8], A[8];
};

__device__ __forceinline__ void load_group(ParamGroup &pg, const_f32_ptr p, uint32_t g) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        pg.w[j] = p[(size_t)g * 16 + 2 * j];
        pg.A[j] = p[(size_t)g * 16 + 2 * j + 1];
    }
}

// A wave sums at most 2^8 groups = 2048 partials (chunk <= 8192 per workgroup): 9 carry levels.
// The levels are separate named arrays, not one 2-D array: hipcc otherwise merges the per-level
// stores into one dynamically indexed store and the whole table drops to scratch memory.
template <int I, int N, class Fn>
__device__ __forceinline__ void static_for(Fn &&fn) {   // compile-time indices: nothing left to index dynamically
    if constexpr (I < N) {
        fn(std::integral_constant<int, I>{});
        static_for<I + 1, N>(fn);
    }
}

template <int F>
using Lvl = float (&)[F];
#define FR_LEVELS_DECL Lvl<F> s0, Lvl<F> s1, Lvl<F> s2, Lvl<F> s3, Lvl<F> s4, Lvl<F> s5, Lvl<F> s6, Lvl<F> s7, Lvl<F> s8
#define FR_LEVELS_PASS s0, s1, s2, s3, s4, s5, s6, s7, s8

template <int F, bool FAST, bool EXACT>
__device__ __forceinline__ void bank_group(const ParamGroup &pg, uint32_t g,
                                           const float (&t)[F], FR_LEVELS_DECL) {
    float v[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
        float l0 = bank_leaf<FAST, EXACT>(t[f], pg.w[0], pg.A[0]);
        float l1 = bank_leaf<FAST, EXACT>(t[f], pg.w[1], pg.A[1]);
        float l2 = bank_leaf<FAST, EXACT>(t[f], pg.w[2], pg.A[2]);
        float l3 = bank_leaf<FAST, EXACT>(t[f], pg.w[3], pg.A[3]);
        float l4 = bank_leaf<FAST, EXACT>(t[f], pg.w[4], pg.A[4]);
        float l5 = bank_leaf<FAST, EXACT>(t[f], pg.w[5], pg.A[5]);
        float l6 = bank_leaf<FAST, EXACT>(t[f], pg.w[6], pg.A[6]);
        float l7 = bank_leaf<FAST, EXACT>(t[f], pg.w[7], pg.A[7]);
        v[f] = ((l0 + l1) + (l2 + l3)) + ((l4 + l5) + (l6 + l7));
    }
    // binary-counter carry: level k holds the finished left sibling of height k (wave-uniform branches);
    // the chain always stops at level `levels` at the latest because g < ngroups = 2^levels
#define FR_CARRY(K, SK)                                                    \
    if (((g >> K) & 1u) == 0u) {   /* g < 2^levels: bit `levels` is 0 */    \
        static_for<0, F>([&](auto f) { SK[f] = v[f]; });                   \
        return;                                                            \
    }                                                                      \
    static_for<0, F>([&](auto f) { v[f] = SK[f] + v[f]; });
    FR_CARRY(0u, s0) FR_CARRY(1u, s1) FR_CARRY(2u, s2) FR_CARRY(3u, s3) FR_CARRY(4u, s4)
    FR_CARRY(5u, s5) FR_CARRY(6u, s6) FR_CARRY(7u, s7)
#undef FR_CARRY
#pragma unroll
    for (int f = 0; f < F; ++f) s8[f] = v[f];
}

// (Fetching a PAIR of parameter groups ahead instead of one -- for launches that leave a SIMD only a few waves to hide a
//  scalar load behind -- was built and measured SLOWER everywhere: 64 x 4096, T = 64 7.5 -> 8.4 us, 256 10.6 -> 13.3,
//  512 17.8 -> 20.1, 1024 29.3 -> 33.0; the 32 extra SGPRs take these kernels to the register limit.
//  profiles/r02_short_calls.txt.)
// `first`: group 0 already requested by the caller (short calls ask for it before they wait for their time row).
template <int F, bool FAST, bool EXACT>
__device__ __forceinline__ void bank_wave_sum(const float *params, uint32_t ngroups, uint32_t levels,
                                              const float (&t)[F], float (&res)[F], const ParamGroup *first = nullptr) {
    float s0[F], s1[F], s2[F], s3[F], s4[F], s5[F], s6[F], s7[F], s8[F];
#pragma unroll
    for (int f = 0; f < F; ++f)
        s0[f] = s1[f] = s2[f] = s3[f] = s4[f] = s5[f] = s6[f] = s7[f] = s8[f] = 0.0f;

    const_f32_ptr p = (const_f32_ptr)params;
    // two parameter groups in flight: the scalar load of group g+1 is issued before group g's math
    ParamGroup pa, pb;
    if (first) pa = *first;
    else load_group(pa, p, 0);
    // (scalar loads return out of order, so the only usable wait is lgkmcnt(0): wait for the group
    // about to be consumed FIRST, then issue the next load so it flies under this group's ~120 VALU ops)
    for (uint32_t g = 0; g < ngroups; g += 2) {
        const bool has_b = g + 1 < ngroups;
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): pa has landed
        if (has_b) load_group(pb, p, g + 1);
        bank_group<F, FAST, EXACT>(pa, g, t, FR_LEVELS_PASS);
        if (has_b) {
            __builtin_amdgcn_s_waitcnt(0xC07F);   // pb has landed
            if (g + 2 < ngroups) load_group(pa, p, g + 2);
            bank_group<F, FAST, EXACT>(pb, g + 1, t, FR_LEVELS_PASS);
        }
    }
    // after the last group (all ones) the carry chain stopped at level `levels`
#pragma unroll
    for (int f = 0; f < F; ++f) {
        float r = s8[f];
        r = levels == 7u ? s7[f] : r;
        r = levels == 6u ? s6[f] : r;
        r = levels == 5u ? s5[f] : r;
        r = levels == 4u ? s4[f] : r;
        r = levels == 3u ? s3[f] : r;
        r = levels == 2u ? s2[f] : r;
        r = levels == 1u ? s1[f] : r;
        r = levels == 0u ? s0[f] : r;
        res[f] = r;
    }
}

// The sign of a zero sum.  An RN sum tree yields -0 iff every leaf is -0 (x + (-x) and (+0) + (-0) are +0), so
// when a workgroup's result holds a zero only that AND over its leaves is needed, never a recomputation.
// The AND is order-free, so here lanes run over PARTIALS (coalesced float2 loads), unlike the hot loop.
// Returns, for this thread's share of partials [0, n), whether all leaves at time t are exactly -0.0 in the
// graph's arithmetic (product-form leaf, general fract: bit-identical to the graph for every input).
__device__ __forceinline__ bool leaves_all_negzero(const float2 *params, uint32_t n, float t, uint32_t tid, uint32_t nthreads) {
    bool ok = true;
    for (uint32_t k = tid; k < n && ok; k += nthreads) {
        float2 p = params[k];
        ok = __float_as_uint(bank_leaf<false, true>(t, p.x, p.y)) == 0x80000000u;
    }
    return ok;
}

// The same question for all 64 frames of a tile at once, for tiles whose results are mostly zeros (a silent voice:
// every amplitude 0; partials beyond 2^23 cycles): lanes over frames and parameters through the scalar cache like
// the hot loop, each wave over its own share of the partials.  Returns per lane whether every leaf of the share is
// exactly -0.0 (AND and OR of the bit patterns both equal to the sign bit).  Not inlined: its registers must not
// disturb the hot loop's allocation (an inlined second loop made the kernel 1.6x slower, profiles/r01_bank_variants.txt).
template <bool FAST>
__device__ __attribute__((noinline)) bool wave_leaves_all_negzero(const float *params, uint32_t ngroups, float t, unsigned long long lanes) {
    // `lanes`: the frames of the tile whose answer is wanted (those whose sum came out zero).  A lane's answer is
    // settled as soon as it meets one leaf that is not -0, so the scan stops once that has happened in every wanted
    // lane -- for a silent voice (amplitudes 0: leaves are +-0 with t-dependent signs; or every t*w beyond 2^23: all
    // leaves +0) that is after the first pair of groups, and the voice costs one pass like a sounding one, not two.
    const_f32_ptr p = (const_f32_ptr)params;
    const bool wanted = (lanes >> (threadIdx.x & 63u)) & 1ull;
    uint32_t all_and = 0xFFFFFFFFu, all_or = 0u;
    ParamGroup pa, pb;
    load_group(pa, p, 0);
    auto fold = [&](const ParamGroup &pg) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            uint32_t b = __float_as_uint(bank_leaf<FAST, true>(t, pg.w[j], pg.A[j]));
            all_and &= b;
            all_or |= b;
        }
    };
    for (uint32_t g = 0; g < ngroups; g += 2) {
        const bool has_b = g + 1 < ngroups;
        __builtin_amdgcn_s_waitcnt(0xC07F);
        if (has_b) load_group(pb, p, g + 1);
        fold(pa);
        if (has_b) {
            __builtin_amdgcn_s_waitcnt(0xC07F);
            if (g + 2 < ngroups) load_group(pa, p, g + 2);
            fold(pb);
        }
        if (__ballot(wanted && all_and == 0x80000000u && all_or == 0x80000000u) == 0ull) {
            __builtin_amdgcn_s_waitcnt(0xC07F);   // (a prefetched group may still be landing in pa)
            return false;
        }
    }
    return all_and == 0x80000000u && all_or == 0x80000000u;
}

__device__ __forceinline__ float bank_time(const BankArgs &a, uint64_t ti) {
    return (ti >= a.time_skip && ti - a.time_skip < a.time_valid) ? a.time[ti - a.time_skip] : 0.0f;
}
__device__ __forceinline__ uint64_t bank_out_index(const BankArgs &a, uint64_t ti) {
    return a.ring_mask ? ((a.ring_t0 + ti) & a.ring_mask) : ti;
}

// MODE 0: every leaf in the product form (always exact).
// MODE 1: FMA-form leaves (5 ops + 1 add per partial-frame); where the workgroup's combined result is a
//         zero, its sign is settled by leaves_all_negzero (rare: t*w integral for every partial, e.g. t = 0).
// MODE 2: FMA-form leaves without the sign repair -- diagnostic only (tools/bank_bench.hip).
// (Recomputing flagged tiles with the product-form loop inside the same kernel was tried first: with a second
//  copy of the hot loop inlined, register allocation degrades and the kernel runs 1.6x slower;
//  profiles/r01_bank_variants.txt.)
// NW = waves per workgroup (4 or 8): a wave is the unit of work that cannot be split further, so more, smaller
// waves shorten the kernel's tail at a given call size (measured: profiles/r01_bank_variants.txt).
// FLAGS: publish row-completion flags to the host (BankArgs::host_flags) -- a separate instantiation, so that the few
// scalar registers it needs never touch the occupancy of the ordinary launches.
template <int F, int MODE, int NW, bool FLAGS = false>
__global__ void __launch_bounds__(64 * NW) bank_kernel(BankArgs a, uint32_t tiles, uint32_t nblocks) {
    // XCD-aware order: blocks b and b+8 share an XCD (round-robin dispatch), so give each XCD a
    // contiguous range of (voice, chunk, tile) work: its L2 then sees 1/8 of the parameter streams.
    uint32_t b = blockIdx.x;
    uint32_t lid = (nblocks % 8u == 0u) ? (b % 8u) * (nblocks / 8u) + b / 8u : b;
    const uint32_t nchunks = 1u << (a.log2_p - a.chunk_log2);
    const uint32_t vc = lid / tiles;                  // voice * nchunks + chunk
    const uint32_t tile = lid - vc * tiles;
    const uint32_t voice = vc >> (a.log2_p - a.chunk_log2);
    const uint32_t chunk = vc & (nchunks - 1u);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    FR_DIAG_MARK(0);
    FR_DIAG_MARK(3);
    const uint64_t t0 = (uint64_t)tile * (64u * F);
    float t[F];
    bool nonneg = true;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        uint64_t ti = t0 + (uint32_t)f * 64u + lane;
        t[f] = bank_time(a, ti);
        nonneg = nonneg && (t[f] >= 0.0f) && (t[f] <= 4294967296.0f);
        // the call's time row doubles as this slot's input history (reference.rs:70): one workgroup
        // column appends it, which saves a separate copy kernel on the stream (only with time_skip == 0)
        if (a.hist_dst && vc == 0u && wave == 0u && ti < a.time_valid) a.hist_dst[ti] = t[f];
    }
    const bool fast = a.fast_ok && __all(nonneg);   // then every x = t*w is in [0, 2^64]: finite, >= 0

    const uint32_t Pc = 1u << a.chunk_log2;           // partials per workgroup, 8*NW <= Pc <= 2048*NW
    const uint32_t Pw = Pc / NW;                      // partials per wave
    const float2 *cparams = a.params + ((size_t)voice << a.log2_p) + (size_t)chunk * Pc;
    const float *params = (const float *)(cparams + (size_t)wave * Pw);
    const uint32_t ngroups = Pw >> 3;
    const uint32_t levels = a.chunk_log2 - 3u - (NW == 8 ? 3u : NW == 4 ? 2u : NW == 2 ? 1u : 0u);   // log2(ngroups) <= 8

    float res[F];
    constexpr bool EXACT = (MODE == 0);
    if (fast) bank_wave_sum<F, true, EXACT>(params, ngroups, levels, t, res);
    else bank_wave_sum<F, false, EXACT>(params, ngroups, levels, t, res);
    FR_DIAG_MARK(1);

    __shared__ float sm[NW][F][64];
    __shared__ unsigned long long zmask[F];
#pragma unroll
    for (int f = 0; f < F; ++f) sm[wave][f][lane] = res[f];
    __syncthreads();
    FR_DIAG_MARK(2);
    // one chunk: straight to the voice's output row; else to the workspace [chunk][voice][t]
    const bool direct = nchunks == 1u;
    float *orow = direct ? a.out + (size_t)a.rows[voice] * a.out_stride
                         : a.ws + ((size_t)chunk * a.n_voices + voice) * a.n_times;
    if (wave == 0) {
#pragma unroll
        for (int f = 0; f < F; ++f) {
            uint64_t ti = t0 + (uint32_t)f * 64u + lane;
            float r = sm[0][f][lane];
            if (NW >= 2) r = r + sm[1 % NW][f][lane];
            if (NW >= 4) r = r + (sm[2 % NW][f][lane] + sm[3 % NW][f][lane]);
            if (NW == 8) r = r + ((sm[4 % NW][f][lane] + sm[5 % NW][f][lane]) + (sm[6 % NW][f][lane] + sm[7 % NW][f][lane]));
            bool live = ti < a.n_times;
            // Streaming store: nothing re-reads it here, and when the row lives in page-locked HOST memory (fr_host_register)
            // the wave is released ~9 us/launch sooner.  FLAGS: the row is read by the host BEFORE the launch ends, as soon as
            // its flag arrives, so the store must be a system-scope one whose acknowledgement means "visible to the host"
            // (a streaming store is acknowledged earlier: the flag overtook the data, tools/host_stream_soak.py).
            if (live) {
                float *dst = &orow[direct ? bank_out_index(a, ti) : ti];
                if (FLAGS) __hip_atomic_store(dst, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                else __builtin_nontemporal_store(r, dst);
            }
            if (MODE == 1) {
                unsigned long long m = __ballot(live && r == 0.0f);
                if (lane == 0) zmask[f] = m;
            }
        }
    }
    if (MODE == 1) {
        __syncthreads();
#pragma unroll
        for (int f = 0; f < F; ++f) {
            unsigned long long m = zmask[f];          // workgroup-uniform
            if (__builtin_popcountll(m) > 4) {        // many zeros in this tile: settle all 64 frames in one pass
                bool mine = fast ? wave_leaves_all_negzero<true>(params, ngroups, t[f], m)
                                 : wave_leaves_all_negzero<false>(params, ngroups, t[f], m);
                sm[wave][f][lane] = mine ? 1.0f : 0.0f;   // (the sums in sm were consumed before the barrier above)
                __syncthreads();
                if (wave == 0 && ((m >> lane) & 1ull)) {
                    bool all = true;
#pragma unroll
                    for (int w = 0; w < NW; ++w) all = all && sm[w][f][lane] != 0.0f;
                    uint64_t ti = t0 + (uint32_t)f * 64u + lane;
                    float *dst = &orow[direct ? bank_out_index(a, ti) : ti];
                    if (FLAGS) __hip_atomic_store(dst, all ? -0.0f : 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    else *dst = all ? -0.0f : 0.0f;
                }
                __syncthreads();
                continue;
            }
            while (m) {
                uint32_t l = (uint32_t)__builtin_ctzll(m);
                m &= m - 1;
                uint64_t ti = t0 + (uint32_t)f * 64u + l;
                float tz = bank_time(a, ti);
                int all = __syncthreads_and(leaves_all_negzero(cparams, Pc, tz, threadIdx.x, 64u * NW) ? 1 : 0);
                if (threadIdx.x == 0) {
                    float *dst = &orow[direct ? bank_out_index(a, ti) : ti];
                    if (FLAGS) __hip_atomic_store(dst, all ? -0.0f : 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    else *dst = all ? -0.0f : 0.0f;
                }
            }
        }
    }
    // Row-completion flag (the host entry point copies finished rows while the launch is still running).  Every output
    // store of this workgroup was issued by wave 0; once they are acknowledged one lane counts the tile in, and the
    // workgroup that brings a voice's count to `tiles` publishes the row's flag to the host (system-scope release).
    if (FLAGS && a.host_flags && direct && wave == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0u) {
            const uint32_t old = __hip_atomic_fetch_add(a.row_done + voice, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old == tiles - 1u) {
                __hip_atomic_store(a.row_done + voice, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
                __hip_atomic_store(a.host_flags + a.rows[voice], a.flag_value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
}

// Many small voices (<= 256 partials each): one workgroup per (batch of voices, tile of frames); every wave sums WHOLE
// voices, `voices_per_wave` of them one after the other, with the same inner loop.  Nothing is shared between waves:
// no LDS, no barriers; the tile's time values are loaded once and stay in registers for all the wave's voices.  (With
// a quarter of a 32-partial voice per wave the fixed cost of a workgroup -- time loads, one exposed parameter load,
// LDS hand-over, barrier -- outweighs its 8 leaves: 2.1 T partial-frames/s.)
template <int F, int MODE>
__global__ void __launch_bounds__(256) bank_multi_kernel(BankArgs a, uint32_t tiles, uint32_t nblocks) {
    uint32_t b = blockIdx.x;
    uint32_t lid = (nblocks % 8u == 0u) ? (b % 8u) * (nblocks / 8u) + b / 8u : b;
    const uint32_t vb = lid / tiles, tile = lid - vb * tiles;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t t0 = (uint64_t)tile * (64u * F);
    float t[F];
    bool nonneg = true;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        uint64_t ti = t0 + (uint32_t)f * 64u + lane;
        t[f] = bank_time(a, ti);
        nonneg = nonneg && (t[f] >= 0.0f) && (t[f] <= 4294967296.0f);
        if (a.hist_dst && vb == 0u && wave == 0u && ti < a.time_valid) a.hist_dst[ti] = t[f];
    }
    const bool fast = a.fast_ok && __all(nonneg);
    const uint32_t ngroups = 1u << (a.log2_p - 3u), levels = a.log2_p - 3u;
    const uint32_t v0 = (vb * 4u + wave) * a.voices_per_wave;
    constexpr bool EXACT = (MODE == 0);
    for (uint32_t j = 0; j < a.voices_per_wave; ++j) {
        const uint32_t voice = v0 + j;
        if (voice >= a.n_voices) break;                      // wave-uniform
        const float2 *vparams = a.params + ((size_t)voice << a.log2_p);
        float res[F];
        if (fast) bank_wave_sum<F, true, EXACT>((const float *)vparams, ngroups, levels, t, res);
        else bank_wave_sum<F, false, EXACT>((const float *)vparams, ngroups, levels, t, res);
        float *orow = a.out + (size_t)a.rows[voice] * a.out_stride;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const uint64_t ti = t0 + (uint32_t)f * 64u + lane;
            const bool live = ti < a.n_times;
            if (live) orow[bank_out_index(a, ti)] = res[f];
            if (MODE == 1) {   // sign of exact zeros, as in bank_kernel, within the wave
                unsigned long long zm = __ballot(live && res[f] == 0.0f);
                if (zm == 0ull) continue;
                if (__builtin_popcountll(zm) > 4) {
                    const bool all = fast ? wave_leaves_all_negzero<true>((const float *)vparams, ngroups, t[f], zm)
                                          : wave_leaves_all_negzero<false>((const float *)vparams, ngroups, t[f], zm);
                    if ((zm >> lane) & 1ull) orow[bank_out_index(a, ti)] = all ? -0.0f : 0.0f;
                    continue;
                }
                while (zm) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(zm);
                    zm &= zm - 1;
                    const uint64_t tz_i = t0 + (uint32_t)f * 64u + l;
                    const float tz = bank_time(a, tz_i);
                    const bool all = __all(leaves_all_negzero(vparams, 1u << a.log2_p, tz, lane, 64u));
                    if (lane == 0u) orow[bank_out_index(a, tz_i)] = all ? -0.0f : 0.0f;
                }
            }
        }
    }
}

// Short calls (fewer frames than half a wave has lanes): time-major lanes would idle, so here lanes run over
// PARTIALS -- the layout the north star sketches: coalesced float2 loads of each partial's {w, A4} (held in
// registers for the call's frames), a wavefront-shuffle butterfly for the per-voice mix, LDS for the 4 waves.
// The butterfly IS the graph's balanced tree: at step m lane i adds the sub-tree sum of lanes i^m, and f32 add is
// bitwise commutative, so after 6 steps every lane holds the tree-ordered sum of its wave's 64 consecutive
// partials.  A workgroup covers 256 consecutive partials of one voice; chunks combine with bank_combine_kernel.
constexpr uint32_t SMALL_MAX_FRAMES = 32;   // capacity of the kernel; bank_shape uses it for T <= 2 only (measured)

__global__ void __launch_bounds__(256) bank_small_kernel(BankArgs a) {
    const uint32_t chunk = blockIdx.x, voice = blockIdx.y;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t nchunks = 1u << (a.log2_p - 8u);
    const float2 prm = a.params[((size_t)voice << a.log2_p) + (size_t)chunk * 256u + threadIdx.x];
    __shared__ float sm[4][SMALL_MAX_FRAMES];
    __shared__ uint32_t zmask;
    for (uint32_t ti = 0; ti < (uint32_t)a.n_times; ++ti) {
        const float t = bank_time(a, ti);                                  // wave-uniform
        const bool fast = a.fast_ok && t >= 0.0f && t <= 4294967296.0f;
        float v = fast ? bank_leaf<true, false>(t, prm.x, prm.y) : bank_leaf<false, false>(t, prm.x, prm.y);
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
        if (lane == 0) sm[wave][ti] = v;
    }
    if (threadIdx.x == 0) zmask = 0u;
    __syncthreads();
    const bool direct = nchunks == 1u;
    float *orow = direct ? a.out + (size_t)a.rows[voice] * a.out_stride
                         : a.ws + ((size_t)chunk * a.n_voices + voice) * a.n_times;
    if (threadIdx.x < a.n_times) {
        const uint32_t ti = threadIdx.x;
        float r = (sm[0][ti] + sm[1][ti]) + (sm[2][ti] + sm[3][ti]);
        orow[direct ? bank_out_index(a, ti) : ti] = r;
        if (r == 0.0f) atomicOr(&zmask, 1u << ti);
    }
    __syncthreads();
    uint32_t zm = zmask;                                                   // workgroup-uniform
    while (zm) {   // the sign of a zero: -0 iff each of this workgroup's 256 leaves is -0 in the graph's arithmetic
        uint32_t ti = (uint32_t)__builtin_ctz(zm);
        zm &= zm - 1;
        float tz = bank_time(a, ti);
        bool neg = __float_as_uint(bank_leaf<false, true>(tz, prm.x, prm.y)) == 0x80000000u;
        int all = __syncthreads_and(neg ? 1 : 0);
        if (threadIdx.x == 0) orow[direct ? bank_out_index(a, ti) : ti] = all ? -0.0f : 0.0f;
    }
}

// Upper levels of the voice's Sum2 tree when a voice was split over several workgroups:
// out[v][t] = TREE_c ws[c][v][t], same binary-counter association, one thread per (v, t).
__global__ void __launch_bounds__(256) bank_combine_kernel(BankArgs a) {
    const uint64_t total = (uint64_t)a.n_voices * a.n_times;
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const uint32_t voice = (uint32_t)(e / a.n_times);
    const uint64_t ti = e - (uint64_t)voice * a.n_times;
    const uint32_t levels = a.log2_p - a.chunk_log2;
    const uint32_t nchunks = 1u << levels;
    constexpr int MAXL = 20;
    float s[MAXL];
#pragma unroll
    for (int k = 0; k < MAXL; ++k) s[k] = 0.0f;
    float result = 0.0f;
    for (uint32_t c = 0; c < nchunks; ++c) {
        float v = a.ws[e + (uint64_t)c * total];
#pragma unroll
        for (int k = 0; k < MAXL; ++k) {
            if ((uint32_t)k == levels) { result = v; break; }
            if (((c >> k) & 1u) == 0u) { s[k] = v; break; }
            v = s[k] + v;
        }
    }
    a.out[(size_t)a.rows[voice] * a.out_stride + bank_out_index(a, ti)] = result;
}


// ---------------------------------------------------------------------------------------------------
// Short calls.  With few (voice, tile) pairs -- a 64-frame block of config C is 64 of them -- the time-major kernel
// above leaves most of the chip idle and each wave walks its 512 partials as a chain of scalar loads: one
// s_load_dwordx16 per 8 partials, ~150 ns each with nothing else on the SIMD to hide it (measured: 11 us per call for
// any call of 8..256 frames, tools/short_call_probe.py).  Here instead
//   * a voice is cut into `nchunks` chunks, one workgroup of NW waves each, so that hundreds of workgroups exist and a
//     wave's chain of parameter loads is a handful of groups long, with several waves per SIMD to overlap them;
//     (staging the chunk's parameters in LDS and reading them back as broadcast ds_read_b128 was built first: a
//     wave-uniform value broadcast to 64 lanes costs the LDS the full 1 KiB of return bandwidth per instruction, and the
//     kernel ran 2-6x SLOWER than the scalar-load form, profiles/r02_short_calls.txt);
//   * lanes still run over frames and a wave still sums its partials in the graph's own association (same bank_group
//     carry chain), the NW wave sums meet in LDS, and the chunk sums meet in HBM: every workgroup stores its 64 chunk
//     sums write-through (sc1), waits for them, and takes a ticket (agent-scope atomic add); the workgroup whose add
//     comes last reads all chunks back (sc1 loads) and adds them in tree order.  One launch, no grid barrier
//     (MI355X_MICROARCH.md, inter-workgroup visibility: sc1 stores -> vmcnt(0) -> one lane's atomic add -> the last
//     adder loads sc1).
// ---------------------------------------------------------------------------------------------------
// one ticket per 128-byte line: neighbouring (voice, tile) pairs would otherwise serialise their atomics on one L2 line
constexpr uint32_t TICKET_STRIDE = BANK_TICKET_STRIDE;

template <int NW>
__global__ void __launch_bounds__(64 * NW) bank_short_kernel(BankArgs a, uint32_t tiles) {
    __shared__ float sm[NW][64];
    __shared__ unsigned long long zshared;
    const uint32_t clog = a.log2_p - a.chunk_log2, nchunks = 1u << clog;
    // (an XCD-aware order like bank_kernel's -- a contiguous (voice, tile, chunk) range per XCD -- measured the same within
    //  noise: 8 x 4096 x 4800 21.7 -> 21.3 us, 16 x 4096 36.8 -> 36.9; profiles/r03_fewvoices.txt)
    const uint32_t chunk = blockIdx.x & (nchunks - 1u);   // the chunks of one (voice, tile) are neighbours in the grid
    const uint32_t vt = blockIdx.x >> clog;
    const uint32_t voice = vt / tiles, tile = vt - voice * tiles;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t ti = (uint64_t)tile * 64u + lane;
    const bool live = ti < a.n_times;
    const uint32_t Pc = 1u << a.chunk_log2;
    const uint32_t Pw = Pc / NW, ngroups = Pw >> 3;
    uint32_t levels = 0;
    while ((1u << levels) < ngroups) ++levels;
    const float *mine = (const float *)(a.params + ((size_t)voice << a.log2_p) + (size_t)chunk * Pc + (size_t)wave * Pw);
    FR_DIAG_MARK(0);
    FR_DIAG_MARK(3);
    ParamGroup first;                                      // requested BEFORE the time row: the two trips to memory overlap
    load_group(first, (const_f32_ptr)mine, 0);
    const float t = bank_time(a, ti);
    if (a.hist_dst && voice == 0u && chunk == 0u && wave == 0u && ti < a.time_valid) a.hist_dst[ti] = t;   // (every tile of voice 0)
    const bool fast = a.fast_ok && __all(t >= 0.0f && t <= 4294967296.0f);   // the same 64 frames in every wave
    const float tt[1] = {t};
    float r_wave[1];
    if (fast) bank_wave_sum<1, true, false>(mine, ngroups, levels, tt, r_wave, &first);
    else bank_wave_sum<1, false, false>(mine, ngroups, levels, tt, r_wave, &first);
    FR_DIAG_MARK(1);
    sm[wave][lane] = r_wave[0];
    __syncthreads();
    FR_DIAG_MARK(2);
    float r = 0.0f;
    if (wave == 0u) {   // the NW wave sums in tree order: adjacent pairs, level by level
        float s[NW];
        static_for<0, NW>([&](auto w) { s[w] = sm[w][lane]; });
        static_for<0, NW / 2>([&](auto i) { s[i] = s[2 * i] + s[2 * i + 1]; });
        if constexpr (NW >= 4) static_for<0, NW / 4>([&](auto i) { s[i] = s[2 * i] + s[2 * i + 1]; });
        if constexpr (NW >= 8) static_for<0, NW / 8>([&](auto i) { s[i] = s[2 * i] + s[2 * i + 1]; });
        if constexpr (NW >= 16) static_for<0, NW / 16>([&](auto i) { s[i] = s[2 * i] + s[2 * i + 1]; });
        r = s[0];
        const unsigned long long z = __ballot(live && r == 0.0f);
        if (lane == 0u) zshared = z;
    }
    __syncthreads();
    const unsigned long long zm = zshared;                // workgroup-uniform
    if (zm != 0ull) {   // the sign of a zero chunk sum: -0 iff every leaf of the chunk is -0 in the graph's arithmetic
        const bool ok = fast ? wave_leaves_all_negzero<true>(mine, ngroups, t, zm) : wave_leaves_all_negzero<false>(mine, ngroups, t, zm);
        sm[wave][lane] = ok ? 1.0f : 0.0f;
        __syncthreads();
        if (wave == 0u && ((zm >> lane) & 1ull)) {
            bool all = true;
            static_for<0, NW>([&](auto w) { all = all && sm[w][lane] != 0.0f; });
            r = all ? -0.0f : 0.0f;
        }
    }
    if (wave != 0u) return;
    float *orow = a.out + (size_t)a.rows[voice] * a.out_stride;
    if (nchunks == 1u) {
        if (live) orow[bank_out_index(a, ti)] = r;
        return;
    }
    // publish this chunk's sums, take a ticket; the last workgroup of the (voice, tile) to arrive adds the chunks up
    const size_t vstride = (size_t)a.n_voices * a.n_times;
    float *slot = a.ws + (size_t)voice * a.n_times;
    if (live) __hip_atomic_store(slot + (size_t)chunk * vstride + ti, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t old = 0u;
    if (lane == 0u) old = __hip_atomic_fetch_add(a.tickets + (size_t)vt * TICKET_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != nchunks - 1u) return;
    if (live) {
        // binary-counter carry over the chunks (nchunks = 2^clog <= 256): level k holds the finished left sibling of
        // height k; named registers, so nothing is indexed dynamically (no scratch)
        float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f, c4 = 0.0f, c5 = 0.0f, c6 = 0.0f, c7 = 0.0f, c8 = 0.0f;
        for (uint32_t c = 0; c < nchunks; ++c) {
            float v = c == chunk ? r : __hip_atomic_load(slot + (size_t)c * vstride + ti, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            do {
                if (!(c & 1u)) { c0 = v; break; } v = c0 + v;
                if (!(c & 2u)) { c1 = v; break; } v = c1 + v;
                if (!(c & 4u)) { c2 = v; break; } v = c2 + v;
                if (!(c & 8u)) { c3 = v; break; } v = c3 + v;
                if (!(c & 16u)) { c4 = v; break; } v = c4 + v;
                if (!(c & 32u)) { c5 = v; break; } v = c5 + v;
                if (!(c & 64u)) { c6 = v; break; } v = c6 + v;
                if (!(c & 128u)) { c7 = v; break; } v = c7 + v;
                c8 = v;
            } while (0);
        }
        float result = c8;   // after the last chunk (all ones) the chain stopped at level clog
        result = clog == 7u ? c7 : result; result = clog == 6u ? c6 : result; result = clog == 5u ? c5 : result;
        result = clog == 4u ? c4 : result; result = clog == 3u ? c3 : result; result = clog == 2u ? c2 : result;
        result = clog == 1u ? c1 : result;
        orow[bank_out_index(a, ti)] = result;
    }
    if (lane == 0u) __hip_atomic_store(a.tickets + (size_t)vt * TICKET_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
}

template <int NW>
static hipError_t launch_bank_short(const BankArgs &a, hipStream_t s) {
    const uint64_t tiles = (a.n_times + 63) / 64;
    const uint64_t nb = (tiles * a.n_voices) << (a.log2_p - a.chunk_log2);
    if (nb == 0) return hipSuccess;
    if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL((bank_short_kernel<NW>), dim3((uint32_t)nb), dim3(64 * NW), 0, s, a, (uint32_t)tiles);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Block streaming: the short-call kernel as ONE resident launch (kernels.hpp, BankStreamCtl).  Each step of the protocol is
// written once, in this section; the skeleton that calls the steps -- stream_resident_body, of which the twelve resident
// kernels are instantiations -- follows stage_kernel, whose interpreter's types it uses.
//
// A block.  The host rings a doorbell in mapped pinned memory: every word carries a sample and the block's tag.  Wave 0 of
// workgroup 0 polls it (stream_row_wait: one row; stream_in_wait: K rows), republishes the rows to device memory, has them
// acknowledged, then stores n_times and -- acknowledged in between -- seq (stream_next_block).  Thread 0 of every other
// workgroup polls seq.  Every workgroup then renders its (voice, chunk) of the block as bank_short_kernel does
// (stream_render_chunk); the chunk sums of a voice meet through a ticket, the last arriver adds them in tree order
// (stream_hand_over) and so finishes the voice: wave 0 of that workgroup stores the voice's 64 frames to its row or ring
// (stream_store_voice), runs the voice's programs, lane = frame (stream_run_programs), and counts the voice in (stream_finish,
// stream_finish_bus); whoever counts the last voice in writes the block's done tag to the host.
//
// The hand-overs.  No workgroup waits for another one's result and there is no acquire or release inside the block loop: all
// traffic between workgroups is relaxed atomics at agent scope (sc1: served by L2, never by a CU's L1 -- the finisher of a voice
// changes CU from block to block), what goes to the host is stored at system scope, and a wave has its own stores acknowledged
// (s_waitcnt vmcnt(0)) before it takes a ticket, before it reads them back, and before the done tag; the wave that draws the
// last ticket issues its loads after that ticket came back (MI355X_MICROARCH.md, inter-workgroup visibility).  What the rule
// on the host guarantees for programs (streamplan.hpp): a program reads at a delay below 64 frames only the ring its own wave
// has just stored, or a ring an earlier program of the same voice stored; everything else was stored by an earlier block, whose
// done tag the host has seen -- except in the bus segment, which runs after every voice of the block was counted in.
//
// The bounds.  Every polling loop is bounded on the 100 MHz wall clock (s_memrealtime): with no block for `idle_ms` workgroup 0
// publishes STOP and the launch ends itself (friendship_render.h: FR_STREAM_IDLE_MS), whatever a look across PCIe happens to
// cost; the followers' bound outlasts workgroup 0's.
//
// 1024 threads per workgroup: at most 128 VGPRs and no scratch -- the interpreter's registers are LDS columns.  The pieces are
// __forceinline__; what they compile to inside each kernel is compared with the kernels' earlier, separately written text in
// profiles/stream_shared_text.txt and profiles/stream_resident_body.txt (registers, LDS, scratch, and the count of every
// barrier, sleep, clock read, vmcnt(0) and atomic), which is where a change to a piece is checked.
// ---------------------------------------------------------------------------------------------------
constexpr int STREAM_NW = 16;   // waves of a streaming workgroup

// What a workgroup renders in every block of the launch (uniform: lives in SGPRs).
struct StreamWork {
    uint32_t voice;        // the global voice: its chunk sums, its ticket and its programs
    uint32_t bank_voice;   // the voice inside its bank: its parameters and its destination
    uint32_t chunk, clog, nchunks;
    uint32_t ngroups, levels;
    const float *mine;     // this wave's partials
    uint32_t fast_ok;
    const uint32_t *rows;  // the bank's destinations: rings (to_ring) or output rows
    uint32_t to_ring;
};

// Workgroup `local` of a bank whose voices are cut into chunks of 1 << chunk_log2 partials; the bank's first voice is global voice `first_voice`.
__device__ __forceinline__ StreamWork stream_work(const float2 *params, const uint32_t *rows, uint32_t log2_p, uint32_t chunk_log2, uint32_t fast_ok, uint32_t to_ring,
                                                  uint32_t first_voice, uint32_t local, uint32_t wave) {
    StreamWork w;
    w.clog = log2_p - chunk_log2;
    w.nchunks = 1u << w.clog;
    w.chunk = local & (w.nchunks - 1u);   // the chunks of one voice are neighbours in the grid
    w.bank_voice = local >> w.clog;
    w.voice = first_voice + w.bank_voice;
    const uint32_t Pc = 1u << chunk_log2;
    const uint32_t Pw = Pc / STREAM_NW;
    w.ngroups = Pw >> 3;
    w.levels = 0;
    while ((1u << w.levels) < w.ngroups) ++w.levels;
    w.mine = (const float *)(params + ((size_t)w.bank_voice << log2_p) + (size_t)w.chunk * Pc + (size_t)wave * Pw);
    w.fast_ok = fast_ok;
    w.rows = rows;
    w.to_ring = to_ring;
    return w;
}

// Workgroup 0's wait for the next block on the one-row doorbell (BankStreamCtl): lane i polls word i.  The block has arrived
// when every lane holds the same new tag; the row is then republished to device memory (acknowledged before the caller stores
// n_times and seq).  Returns the block's tag (BANK_STREAM_STOP: stop, or no block within the bound).
__device__ __forceinline__ uint32_t stream_row_wait(BankStreamCtl *ctl, BankStreamDev *dev, uint32_t lane, uint32_t seen, unsigned long long idle_ticks, uint32_t &T) {
    uint32_t tag = seen;
    float v = 0.0f;
    bool fresh = false;
    const unsigned long long wait_from = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        const unsigned long long word = __hip_atomic_load(&ctl->row[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        tag = (uint32_t)(word >> 32);
        v = __uint_as_float((uint32_t)word);
        fresh = __all(tag != seen) && (uint32_t)__builtin_amdgcn_readfirstlane(tag) == tag;   // every lane holds the same new tag
        fresh = __all(fresh);
        if (fresh || __builtin_amdgcn_s_memrealtime() - wait_from > idle_ticks) break;
    }
    const uint32_t seq = fresh ? __builtin_amdgcn_readfirstlane(tag) : BANK_STREAM_STOP;   // nobody rang: end
    T = 0;
    if (seq != BANK_STREAM_STOP) {
        T = seq & 0xFFu;
        T = T > 64u ? 64u : T;
        __hip_atomic_store(&dev->row[lane], lane < T ? v : 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    return seq;
}

// The same for a doorbell of K rows (BankStreamInCtl).  One look = the loads of all K rows in flight together, then one wait: a
// word whose tag is new carries its sample with it, so however many rows there are the block costs one trip across PCIe.  The
// block has arrived when every lane of every row holds the same new tag.  `keep(row, sample, T)`: what else workgroup 0 does
// with a row's samples under the same acknowledgement (StreamNoHistory: nothing; StreamHistoryStore: the hist form's history).
struct StreamNoHistory {
    __device__ __forceinline__ void operator()(uint32_t, float, uint32_t) const {}
};
template <uint32_t K, class Keep>
__device__ __forceinline__ uint32_t stream_in_wait(BankStreamInCtl *ctl, BankStreamInDev *dev, uint32_t lane, uint32_t seen, unsigned long long idle_ticks, uint32_t &T,
                                                   const Keep &keep) {
    unsigned long long word[K];
    uint32_t tag = seen;
    bool fresh = false;
    const unsigned long long wait_from = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        static_for<0, K>([&](auto j) { word[j] = __hip_atomic_load(&ctl->rows[j][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); });
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tag = (uint32_t)(word[0] >> 32);
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane(tag);
        bool same = tag != seen && tag == first;
        static_for<1, K>([&](auto j) { same = same && (uint32_t)(word[j] >> 32) == first; });
        fresh = __all(same);
        if (fresh || __builtin_amdgcn_s_memrealtime() - wait_from > idle_ticks) break;
    }
    const uint32_t seq = fresh ? __builtin_amdgcn_readfirstlane(tag) : BANK_STREAM_STOP;
    T = 0;
    if (seq != BANK_STREAM_STOP) {
        T = seq & 0xFFu;
        T = T > 64u ? 64u : T;
        static_for<0, K>([&](auto j) {
            __hip_atomic_store(&dev->rows[j][lane], lane < T ? __uint_as_float((uint32_t)word[j]) : 0.0f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        });
        static_for<0, K>([&](auto j) { keep((uint32_t)j, __uint_as_float((uint32_t)word[j]), T); });
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    return seq;
}

// (launch-uniform row count: one jump, then a loop whose every look is straight-line code)
template <class Keep>
__device__ __forceinline__ uint32_t stream_rows_wait(uint32_t n_rows, BankStreamInCtl *ctl, BankStreamInDev *dev, uint32_t lane, uint32_t seen,
                                                     unsigned long long idle_ticks, uint32_t &T, const Keep &keep) {
    switch (n_rows) {
    case 1: return stream_in_wait<1>(ctl, dev, lane, seen, idle_ticks, T, keep);
    case 2: return stream_in_wait<2>(ctl, dev, lane, seen, idle_ticks, T, keep);
    case 3: return stream_in_wait<3>(ctl, dev, lane, seen, idle_ticks, T, keep);
    case 4: return stream_in_wait<4>(ctl, dev, lane, seen, idle_ticks, T, keep);
    case 5: return stream_in_wait<5>(ctl, dev, lane, seen, idle_ticks, T, keep);
    case 6: return stream_in_wait<6>(ctl, dev, lane, seen, idle_ticks, T, keep);
    case 7: return stream_in_wait<7>(ctl, dev, lane, seen, idle_ticks, T, keep);
    default: return stream_in_wait<8>(ctl, dev, lane, seen, idle_ticks, T, keep);
    }
}

// Every workgroup's wait for the next block.  Wave 0 of workgroup 0 runs `doorbell` (one of the waits above) and publishes what
// it brought: n_times, acknowledged, then seq (the rows were acknowledged by the wait).  Thread 0 of any other workgroup polls
// seq; its bound outlasts workgroup 0's, which ends in a STOP for everybody.  Returns the block's tag and its frames in T.
template <class Dev, class Doorbell>
__device__ __forceinline__ uint32_t stream_next_block(Dev *dev, uint32_t wave, uint32_t lane, uint32_t seen, unsigned long long idle_ticks, uint32_t &s_seq, uint32_t &s_T,
                                                      uint32_t &T, Doorbell &&doorbell) {
    if (blockIdx.x == 0) {
        if (wave == 0u) {
            uint32_t T0 = 0;
            const uint32_t seq = doorbell(T0);
            if (lane == 0u) {
                __hip_atomic_store(&dev->n_times, T0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(&dev->seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (rows and n_times are acknowledged)
                s_seq = seq;
                s_T = T0;
            }
        }
    } else if (threadIdx.x == 0) {
        uint32_t seq = seen;
        const unsigned long long wait_from = __builtin_amdgcn_s_memrealtime();
        for (;;) {
            seq = __hip_atomic_load(&dev->seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seq != seen || __builtin_amdgcn_s_memrealtime() - wait_from > 2ull * idle_ticks + 10000000ull) break;
            __builtin_amdgcn_s_sleep(4);
        }
        if (seq == seen) seq = BANK_STREAM_STOP;
        s_seq = seq;
        s_T = __hip_atomic_load(&dev->n_times, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    T = s_T;
    return s_seq;
}

// One (voice, chunk) of one tile, as bank_short_kernel: lane = frame, `trow` the block's republished time row (its load is
// requested after the first parameter group's, so the two trips to memory overlap).  Returns the chunk's sum in wave 0, a zero
// with the sign the graph's arithmetic gives it; `t` is the lane's time in every wave.  Two barriers, a third when a sum is zero.
__device__ __forceinline__ float stream_render_chunk(const StreamWork &w, const float *trow, bool live, uint32_t wave, uint32_t lane, float (&sm)[STREAM_NW][64],
                                                     unsigned long long &zshared, float &t) {
    constexpr int NW = STREAM_NW;
    ParamGroup first;
    load_group(first, (const_f32_ptr)w.mine, 0);
    t = live ? __hip_atomic_load(&trow[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
    const bool fast = w.fast_ok && __all(t >= 0.0f && t <= 4294967296.0f);
    const float tt[1] = {t};
    float r_wave[1];
    if (fast) bank_wave_sum<1, true, false>(w.mine, w.ngroups, w.levels, tt, r_wave, &first);
    else bank_wave_sum<1, false, false>(w.mine, w.ngroups, w.levels, tt, r_wave, &first);
    sm[wave][lane] = r_wave[0];
    __syncthreads();
    float r = 0.0f;
    if (wave == 0u) {   // the NW wave sums in tree order: adjacent pairs, level by level
        float s[NW];
        static_for<0, NW>([&](auto i) { s[i] = sm[i][lane]; });
        static_for<0, NW / 2>([&](auto i) { s[i] = s[2 * i] + s[2 * i + 1]; });
        static_for<0, NW / 4>([&](auto i) { s[i] = s[2 * i] + s[2 * i + 1]; });
        static_for<0, NW / 8>([&](auto i) { s[i] = s[2 * i] + s[2 * i + 1]; });
        static_for<0, NW / 16>([&](auto i) { s[i] = s[2 * i] + s[2 * i + 1]; });
        r = s[0];
        const unsigned long long z = __ballot(live && r == 0.0f);
        if (lane == 0u) zshared = z;
    }
    __syncthreads();
    const unsigned long long zm = zshared;                // workgroup-uniform
    if (zm != 0ull) {   // the sign of a zero chunk sum: -0 iff every leaf of the chunk is -0 in the graph's arithmetic
        const bool ok = fast ? wave_leaves_all_negzero<true>(w.mine, w.ngroups, t, zm) : wave_leaves_all_negzero<false>(w.mine, w.ngroups, t, zm);
        sm[wave][lane] = ok ? 1.0f : 0.0f;
        __syncthreads();
        if (wave == 0u && ((zm >> lane) & 1ull)) {
            bool all = true;
            static_for<0, NW>([&](auto i) { all = all && sm[i][lane] != 0.0f; });
            r = all ? -0.0f : 0.0f;
        }
    }
    return r;
}

// A SCHEDULE voice (FR_STREAM_GENERAL, kernels.hpp StreamGeneralArgs): gbank_tile for 16 waves.  gbank_group and the depth of
// the evaluation stack are the general voices' own, further down (GB_MAX_DEPTH).
template <bool FAST>
__device__ __forceinline__ float gbank_group(const ParamGroup &pg, uint32_t j, float t);
constexpr uint32_t STREAM_STACK_DEPTH = 16;

// The items of the voice in schedule order, lane = frame.  An item of 2^k >= 16 leaves is a complete sub-tree: the first
// min(16, 2^(k-3)) waves each sum 2^(k-7) groups of 8 (one group below 128 leaves) with the balanced kernel's inner loop, the
// wave sums meet in `sm` and wave 0 adds them in tree order -- adjacent pairs, the ladder of stream_render_chunk, of which an
// item of fewer than 128 leaves takes a lower rung.  One barrier per such item: its condition is the schedule word, uniform
// for the workgroup, and every wave of the workgroup walks every item.  The hand-over is double-buffered as in gbank_tile (item
// i + 2 reuses item i's buffer only after the barrier of item i + 1, which wave 0 reaches after it has read item i's).  Items
// of at most 8 leaves and every merge (v = pop() + v, the tree's own add, left operand on the left) run on wave 0, on its LDS
// stack.  Returns the root in wave 0.
template <bool FAST>
__device__ __forceinline__ float stream_schedule_sum(const float *params, const uint32_t *gmeta, uint32_t nitems, float t, uint32_t wave, uint32_t lane,
                                                     float *stack /* wave 0: [STREAM_STACK_DEPTH][64] + lane */, float (&sm)[2][STREAM_NW][64]) {
    constexpr int NW = STREAM_NW;
    uint32_t sp = 0;
    const_f32_ptr p = (const_f32_ptr)params;
    typedef uint32_t __attribute__((address_space(4))) const *const_u32_ptr;
    const_u32_ptr gm = (const_u32_ptr)gmeta;
    auto finish = [&](float v, uint32_t meta) {        // wave 0 only; (the host validated the schedule: the masks never bite)
        for (uint32_t m = meta >> 4; m != 0u; --m) {   // v = pop() + v
            --sp;
            v = stack[(sp & (STREAM_STACK_DEPTH - 1u)) * 64u] + v;
        }
        stack[(sp & (STREAM_STACK_DEPTH - 1u)) * 64u] = v;
        ++sp;
    };
    uint32_t goff = 0;          // parameter group (8 pairs) the current item starts at
    uint32_t nbig = 0;
    for (uint32_t i = 0; i < nitems; ++i) {
        const uint32_t meta = gm[i];
        const uint32_t k = meta & 15u;
        if (k >= 4u) {          // 16..2048 leaves
            const uint32_t wl = k >= 7u ? 4u : k - 3u;   // log2 of the waves that work on it
            const uint32_t lv = k - 3u - wl;             // ... and of the groups each of them sums
            float(&buf)[NW][64] = sm[nbig & 1u];
            ++nbig;
            if (wave < (1u << wl)) {
                const float tt[1] = {t};
                float res[1];
                bank_wave_sum<1, FAST, false>(params + ((size_t)goff + ((size_t)wave << lv)) * 16u, 1u << lv, lv, tt, res);
                buf[wave][lane] = res[0];
            }
            __syncthreads();    // (uniform: k is the schedule's)
            if (wave == 0u) {   // the ladder; rows of waves that did not work hold whatever they held and reach no rung that is taken
                float s[NW];
                static_for<0, NW>([&](auto j) { s[j] = buf[j][lane]; });
                static_for<0, NW / 2>([&](auto j) { s[j] = s[2 * j] + s[2 * j + 1]; });
                const float a1 = s[0];
                static_for<0, NW / 4>([&](auto j) { s[j] = s[2 * j] + s[2 * j + 1]; });
                const float a2 = s[0];
                static_for<0, NW / 8>([&](auto j) { s[j] = s[2 * j] + s[2 * j + 1]; });
                const float a3 = s[0];
                static_for<0, NW / 16>([&](auto j) { s[j] = s[2 * j] + s[2 * j + 1]; });
                float v = s[0];
                v = wl == 3u ? a3 : v;
                v = wl == 2u ? a2 : v;
                v = wl == 1u ? a1 : v;
                finish(v, meta);
            }
            goff += 1u << (k - 3u);
        } else {
            if (wave == 0u) {   // 1..8 leaves: one group, padding pairs are not leaves
                ParamGroup cur;
                load_group(cur, p, goff);
                __builtin_amdgcn_s_waitcnt(0xC07F);
                finish(gbank_group<FAST>(cur, k, t), meta);
            }
            goff += 1u;
        }
    }
    return wave == 0u ? stack[0] : 0.0f;   // a validated schedule leaves exactly the root
}

// Whether every leaf of this wave's share of the voice is -0 at the lanes `zm`, shaped like the sum: the waves that summed an
// item scan it, wave 0 the leaves of the small items; a wave without a share answers true.
template <bool FAST>
__device__ __forceinline__ bool stream_schedule_negzero(const float *params, const uint32_t *gmeta, uint32_t nitems, float t, uint32_t wave, unsigned long long zm) {
    typedef uint32_t __attribute__((address_space(4))) const *const_u32_ptr;
    const_u32_ptr gm = (const_u32_ptr)gmeta;
    bool ok = true;
    uint32_t goff = 0;
    for (uint32_t i = 0; i < nitems; ++i) {
        const uint32_t k = gm[i] & 15u;
        if (k >= 4u) {
            const uint32_t wl = k >= 7u ? 4u : k - 3u;
            const uint32_t lv = k - 3u - wl;
            if (wave < (1u << wl)) {
                const bool item = wave_leaves_all_negzero<FAST>(params + ((size_t)goff + ((size_t)wave << lv)) * 16u, 1u << lv, t, zm);
                ok = ok && item;
            }
            goff += 1u << (k - 3u);
        } else {
            if (wave == 0u) {
                for (uint32_t j = 0; j < (1u << k); ++j) {
                    const float2 pr = ((const float2 *)params)[(size_t)goff * 8u + j];   // wave-uniform address
                    ok = ok && __float_as_uint(bank_leaf<FAST, true>(t, pr.x, pr.y)) == 0x80000000u;
                }
            }
            goff += 1u;
        }
    }
    return ok;
}

// One schedule voice of one block: the time row as stream_render_chunk reads it, the fast path per workgroup (every wave holds
// the same 64 frames), the sum, and where a live lane's root is zero its sign: -0 iff every leaf of the voice is -0 in the
// graph's arithmetic, the 16 waves' answers ANDed through LDS.  Returns the root in wave 0; `t` is the lane's time in every wave.
// Barriers: one per item of >= 16 leaves, one for the zero mask, a last one when a root is zero -- all under conditions that are
// uniform for the workgroup.
__device__ __forceinline__ float stream_render_schedule(const float *params, const uint32_t *gmeta, uint32_t nitems, uint32_t fast_ok, const float *trow, bool live, uint32_t wave,
                                                        uint32_t lane, float (&sm)[2][STREAM_NW][64], float (&stack_mem)[STREAM_STACK_DEPTH][64], unsigned long long &zshared,
                                                        float &t) {
    constexpr int NW = STREAM_NW;
    t = live ? __hip_atomic_load(&trow[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
    const bool fast = fast_ok && __all(t >= 0.0f && t <= 4294967296.0f);
    float *stack = &stack_mem[0][lane];
    float r = fast ? stream_schedule_sum<true>(params, gmeta, nitems, t, wave, lane, stack, sm) : stream_schedule_sum<false>(params, gmeta, nitems, t, wave, lane, stack, sm);
    if (wave == 0u) {
        const unsigned long long z = __ballot(live && r == 0.0f);
        if (lane == 0u) zshared = z;
    }
    __syncthreads();
    const unsigned long long zm = zshared;                // workgroup-uniform
    if (zm != 0ull) {
        const bool ok = fast ? stream_schedule_negzero<true>(params, gmeta, nitems, t, wave, zm) : stream_schedule_negzero<false>(params, gmeta, nitems, t, wave, zm);
        sm[0][wave][lane] = ok ? 1.0f : 0.0f;             // (every wave is past the last hand-over of the sum: zshared's barrier)
        __syncthreads();
        if (wave == 0u && ((zm >> lane) & 1ull)) {
            bool all = true;
            static_for<0, NW>([&](auto i) { all = all && sm[0][i][lane] != 0.0f; });
            r = all ? -0.0f : 0.0f;
        }
    }
    return r;
}

// A LEAF BANK (FR_STREAM_LEAVES, kernels.hpp StreamLeafArgs, where the argument stands): one (voice, chunk) of one block of
// compiled voices, the leaf interpreted.  Lane = frame; the wave walks its 1/16 of the chunk's partials, and per partial runs
// the bank's leaf program on its own register columns lr[register][lane] in LDS (a wave's LDS accesses complete in program
// order, and no other wave touches its columns: no barrier inside).  What is uniform -- the instruction words, the partial's row
// of the parameter table -- comes through the scalar cache (constant address space); a register and a staged row are LDS reads
// at the lane's column.  Every arithmetic op is prim_binop's, separately rounded; no fast path, no fract body.
// TR (the track forms, kernels.hpp StreamTrackArgs): the operand kind is decoded with 3 bits and kind 4 is a track row's value at
// the lane's frame, which the wave parked in column v of `tp` before it started the partial (stream_render_leaves).
template <bool TR>
__device__ __forceinline__ float stream_leaf_operand(uint32_t kind, uint32_t v, const_f32_ptr prow, uint32_t k, const float (&lr)[BANK_STREAM_LEAF_REGS][64],
                                                     const float (&lin)[BANK_STREAM_ROWS][64], [[maybe_unused]] const float (*tp)[64], uint32_t lane) {
    if constexpr (TR)
        if (kind >= 4u) return tp[v & (BANK_STREAM_LEAF_TRACKS - 1u)][lane];
    switch (kind) {   // (uniform)
    case 0u: return lr[v & (BANK_STREAM_LEAF_REGS - 1u)][lane];
    case 1u: return v < k ? prow[v] : 0.0f;   // (the host numbered the columns below k: the test never bites)
    case 2u: return __uint_as_float(v);
    default: return lin[v & (BANK_STREAM_ROWS - 1u)][lane];
    }
}
typedef uint32_t __attribute__((address_space(4))) const *const_leaf_ptr;   // the instruction words: uniform, SMEM loads
template <bool TR>
__device__ __forceinline__ float stream_leaf(const StreamLeafArgs::Bank &lb, const_f32_ptr prow, float (&lr)[BANK_STREAM_LEAF_REGS][64],
                                             const float (&lin)[BANK_STREAM_ROWS][64], const float (*tp)[64], uint32_t lane, bool sparkle) {
    constexpr uint32_t KIND = TR ? 7u : 3u;
    const_leaf_ptr ins = (const_leaf_ptr)lb.instrs;
    const uint32_t n = lb.n_instr < BANK_STREAM_LEAF_INSTRS ? lb.n_instr : BANK_STREAM_LEAF_INSTRS;
    float v = 0.0f;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t head = ins[4u * i], a = ins[4u * i + 1u], b = ins[4u * i + 2u];   // {op | dst << 8 | ka << 16 | kb << 24, a, b, 0}
        const float x = stream_leaf_operand<TR>((head >> 16) & KIND, a, prow, lb.k, lr, lin, tp, lane);
        const float y = stream_leaf_operand<TR>((head >> 24) & KIND, b, prow, lb.k, lr, lin, tp, lane);
        switch (head & 0xFFu) {   // (the interpreter's own cases, each op a constant, as STAGE_ARITH_CASES)
        case OP_SUM2: v = prim_binop(OP_SUM2, x, y, sparkle); break;
        case OP_MUL: v = prim_binop(OP_MUL, x, y, sparkle); break;
        case OP_DIV: v = prim_binop(OP_DIV, x, y, sparkle); break;
        case OP_MOD: v = prim_binop(OP_MOD, x, y, sparkle); break;
        default: v = prim_binop(OP_MIN, x, y, sparkle); break;
        }
        lr[(head >> 8) & (BANK_STREAM_LEAF_REGS - 1u)][lane] = v;
    }
    // (the last instruction's value is the leaf -- its register is the result -- unless the leaf is a bare constant or input)
    return lb.result_kind == 0u ? v : stream_leaf_operand<TR>(lb.result_kind, lb.result, prow, lb.k, lr, lin, tp, lane);
}

// The track rows of ONE partial (the track forms, kernels.hpp StreamTrackArgs, where the argument stands): row q of the partial
// whose parameter row is `prow` is the slot whose bits stand in column cols[q] (a literal column: cols[q] itself).
struct StreamTrackWave {
    const float *staging;
    uint32_t first_slot, rows;
    StreamTrackArgs::Bank tb;
    uint32_t k;
    __device__ __forceinline__ uint32_t slot(uint32_t q, const_f32_ptr prow) const {   // (uniform; q is a constant of the unrolled callers)
        const uint32_t c = tb.cols[q];
        return ((tb.literal >> q) & 1u) ? c : c < k ? __float_as_uint(prow[c]) : 0xFFFFFFFFu;
    }
    // The load: a relaxed system-scope atomic load of the lane's frame -- a trip across PCIe -- when the slot lies inside the
    // ALLOCATION (a launch constant: the address is in bounds whatever the block says); whether the block supplied it is the park's.
    __device__ __forceinline__ float load(uint32_t q, const_f32_ptr prow, uint32_t lane) const {
        if (q >= tb.n) return 0.0f;
        const uint32_t off = slot(q, prow) - first_slot;
        return off < rows ? __hip_atomic_load(staging + (size_t)off * 64u + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0.0f;
    }
    // The park: what jit_track yields -- the loaded value for a slot below the block's limit (and inside the rows the block
    // staged), +0.0 otherwise and for a lane beyond the block.
    __device__ __forceinline__ void park(uint32_t q, const_f32_ptr prow, float v, uint32_t limit, uint32_t block_rows, bool live, float (*tp)[64], uint32_t lane) const {
        if (q >= tb.n) return;
        const uint32_t s = slot(q, prow);
        tp[q][lane] = live && s < limit && s - first_slot < block_rows ? v : 0.0f;
    }
};

// The rows in flight (the track forms): the values of the NEXT partial's track rows, and the block's control word.  The
// constructor issues the loads of partial 0 and of the word; step(j) parks partial j's values in half j & 1 of the wave's
// double buffer -- the wait for the loads stands here --, issues partial j + 1's loads and returns the half.  The other forms'
// object is empty and its step returns null.
template <bool TR>
struct StreamTrackAhead {
    __device__ __forceinline__ StreamTrackAhead(const StreamTrackWave &, const unsigned long long *, const_f32_ptr, uint32_t) {}
    __device__ __forceinline__ const float (*step(const StreamTrackWave &, float (*)[2][BANK_STREAM_LEAF_TRACKS][64], uint32_t, uint32_t, uint32_t, const_f32_ptr, uint32_t, bool,
                                                 uint32_t))[64] { return nullptr; }
};
template <>
struct StreamTrackAhead<true> {
    float n0, n1, n2, n3;
    unsigned long long word;
    __device__ __forceinline__ StreamTrackAhead(const StreamTrackWave &tw, const unsigned long long *block_tracks, const_f32_ptr prow, uint32_t lane) {
        word = __hip_atomic_load(block_tracks, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        n0 = tw.load(0u, prow, lane); n1 = tw.load(1u, prow, lane); n2 = tw.load(2u, prow, lane); n3 = tw.load(3u, prow, lane);
    }
    __device__ __forceinline__ const float (*step(const StreamTrackWave &tw, float (*trk)[2][BANK_STREAM_LEAF_TRACKS][64], uint32_t wave, uint32_t j, uint32_t n,
                                                 const_f32_ptr prow, uint32_t k, bool live, uint32_t lane))[64] {
        float(*tp)[64] = trk[wave][j & 1u];
        const uint32_t limit = __builtin_amdgcn_readfirstlane((uint32_t)word), block_rows = __builtin_amdgcn_readfirstlane((uint32_t)(word >> 32));
        tw.park(0u, prow, n0, limit, block_rows, live, tp, lane); tw.park(1u, prow, n1, limit, block_rows, live, tp, lane);
        tw.park(2u, prow, n2, limit, block_rows, live, tp, lane); tw.park(3u, prow, n3, limit, block_rows, live, tp, lane);
        if (j + 1u < n) {
            const_f32_ptr next = prow + k;
            n0 = tw.load(0u, next, lane); n1 = tw.load(1u, next, lane); n2 = tw.load(2u, next, lane); n3 = tw.load(3u, next, lane);
        }
        return tp;
    }
};

// The chunk: the block's streamed rows staged in LDS (wave j loads row j; row 0 is the time row; a lane beyond the block holds
// +0.0, as the republished rows do), then the leaves summed LITERALLY in the graph's association -- a group of 8 as bank_group
// adds it, the binary-counter carry over the wave's <= 64 groups, the 16 wave sums in tree order through `sm` as
// stream_render_chunk adds them.  Every add is performed, so a zero sum has the graph's sign: no repair pass.  Two barriers,
// both under the workgroup-uniform condition that the bank is a leaf bank.  Returns the chunk's sum in wave 0; `t` is the lane's
// time in every wave.
// TR (the track forms): the wave has the track rows of partial j + 1 in flight while it interprets partial j.  It loads partial
// 0's rows and the block's limit word before the loop; every iteration parks its own rows in its half trk[wave][j & 1] of the
// wave's double buffer -- the wait for the loads stands here, after a whole partial's interpretation --, issues the next
// partial's loads and interprets (StreamTrackAhead).  Named registers n0..n3: nothing is indexed dynamically.
template <bool TR = false>
__device__ __forceinline__ float stream_render_leaves(const StreamWork &w, const StreamBanksArgs::Bank &bk, const StreamLeafArgs::Bank &lb, const BankStreamInDev *dev,
                                                      uint32_t n_rows, bool sparkle, bool live, uint32_t wave, uint32_t lane, float (&sm)[STREAM_NW][64],
                                                      float (&lregs)[STREAM_NW][BANK_STREAM_LEAF_REGS][64], float (&lin)[BANK_STREAM_ROWS][64], float &t,
                                                      [[maybe_unused]] const StreamTrackWave &tw = {}, [[maybe_unused]] const unsigned long long *block_tracks = nullptr,
                                                      [[maybe_unused]] float (*trk)[2][BANK_STREAM_LEAF_TRACKS][64] = nullptr) {
    constexpr int NW = STREAM_NW;
    if (wave < BANK_STREAM_ROWS)
        lin[wave][lane] = live && wave < n_rows ? __hip_atomic_load(&dev->rows[wave][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
    __syncthreads();
    t = lin[0][lane];
    float(&lr)[BANK_STREAM_LEAF_REGS][64] = lregs[wave];
    // this wave's partials: 8 * ngroups of them, from partial `first` of the bank's table [voice][P][k]
    const size_t first = ((size_t)w.bank_voice << bk.log2_p) + ((size_t)w.chunk << bk.chunk_log2) + (size_t)wave * (w.ngroups << 3);
    const_f32_ptr prow = (const_f32_ptr)((const float *)bk.params + first * lb.k);
    // ONE binary counter over the wave's partials: level k holds the finished left sibling of height k.  Its levels 0..2 add a group
    // of 8 as ((l0 + l1) + (l2 + l3)) + ((l4 + l5) + (l6 + l7)), the levels above are the carry chain over the groups -- one loop,
    // one copy of the interpreter.  Named registers: nothing is indexed dynamically (no scratch).  j < 512: stream_bank_ok.
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f, c4 = 0.0f, c5 = 0.0f, c6 = 0.0f, c7 = 0.0f, c8 = 0.0f, c9 = 0.0f;
    const uint32_t n = w.ngroups << 3;
    StreamTrackAhead<TR> ahead(tw, block_tracks, prow, lane);
    for (uint32_t j = 0; j < n; ++j) {
        float v = stream_leaf<TR>(lb, prow, lr, lin, ahead.step(tw, trk, wave, j, n, prow, lb.k, live, lane), lane, sparkle);
        prow += lb.k;
        do {
            if (!(j & 1u)) { c0 = v; break; } v = c0 + v;
            if (!(j & 2u)) { c1 = v; break; } v = c1 + v;
            if (!(j & 4u)) { c2 = v; break; } v = c2 + v;
            if (!(j & 8u)) { c3 = v; break; } v = c3 + v;
            if (!(j & 16u)) { c4 = v; break; } v = c4 + v;
            if (!(j & 32u)) { c5 = v; break; } v = c5 + v;
            if (!(j & 64u)) { c6 = v; break; } v = c6 + v;
            if (!(j & 128u)) { c7 = v; break; } v = c7 + v;
            if (!(j & 256u)) { c8 = v; break; } v = c8 + v;
            c9 = v;
        } while (0);
    }
    const uint32_t top = w.levels + 3u;   // after the last partial (all ones) the chain stopped at level log2(n)
    float rw = c9;
    rw = top == 8u ? c8 : rw; rw = top == 7u ? c7 : rw; rw = top == 6u ? c6 : rw;
    rw = top == 5u ? c5 : rw; rw = top == 4u ? c4 : rw; rw = top == 3u ? c3 : rw;
    sm[wave][lane] = rw;
    __syncthreads();
    float r = 0.0f;
    if (wave == 0u) {   // the NW wave sums in tree order: adjacent pairs, level by level
        float s[NW];
        static_for<0, NW>([&](auto i) { s[i] = sm[i][lane]; });
        static_for<0, NW / 2>([&](auto i) { s[i] = s[2 * i] + s[2 * i + 1]; });
        static_for<0, NW / 4>([&](auto i) { s[i] = s[2 * i] + s[2 * i + 1]; });
        static_for<0, NW / 8>([&](auto i) { s[i] = s[2 * i] + s[2 * i + 1]; });
        static_for<0, NW / 16>([&](auto i) { s[i] = s[2 * i] + s[2 * i + 1]; });
        r = s[0];
    }
    return r;
}

// Wave 0 hands its chunk sum `r` over: store, acknowledged, then a ticket; the wave whose ticket is the voice's last reads all
// chunks back and adds them in tree order, takes the top of the ladder for this voice's chunk count and resets the ticket for
// the next block.  The chunk sums of all voices share one workspace, [chunk][n_voices][64] by global voice; one ticket per
// voice.  True in the wave that finished the voice, with its frames in `result`.
__device__ __forceinline__ bool stream_hand_over(const StreamWork &w, float *ws, uint32_t *tickets, uint32_t n_voices, uint32_t lane, float r, float &result) {
    result = r;
    if (w.nchunks == 1u) return true;
    const size_t vstride = (size_t)n_voices * 64u;
    float *slot = ws + (size_t)w.voice * 64u;
    __hip_atomic_store(slot + (size_t)w.chunk * vstride + lane, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t old = 0u;
    if (lane == 0u) old = __hip_atomic_fetch_add(tickets + (size_t)w.voice * TICKET_STRIDE, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != w.nchunks - 1u) return false;
    // binary-counter carry over the chunks (nchunks = 2^clog <= 256): level k holds the finished left sibling of height k;
    // named registers, so nothing is indexed dynamically (no scratch)
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f, c4 = 0.0f, c5 = 0.0f, c6 = 0.0f, c7 = 0.0f, c8 = 0.0f;
    for (uint32_t c = 0; c < w.nchunks; ++c) {
        float v = c == w.chunk ? r : __hip_atomic_load(slot + (size_t)c * vstride + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        do {
            if (!(c & 1u)) { c0 = v; break; } v = c0 + v;
            if (!(c & 2u)) { c1 = v; break; } v = c1 + v;
            if (!(c & 4u)) { c2 = v; break; } v = c2 + v;
            if (!(c & 8u)) { c3 = v; break; } v = c3 + v;
            if (!(c & 16u)) { c4 = v; break; } v = c4 + v;
            if (!(c & 32u)) { c5 = v; break; } v = c5 + v;
            if (!(c & 64u)) { c6 = v; break; } v = c6 + v;
            if (!(c & 128u)) { c7 = v; break; } v = c7 + v;
            c8 = v;
        } while (0);
    }
    const uint32_t clog = w.clog;
    result = c8;   // after the last chunk (all ones) the chain stopped at level clog
    result = clog == 7u ? c7 : result; result = clog == 6u ? c6 : result; result = clog == 5u ? c5 : result;
    result = clog == 4u ? c4 : result; result = clog == 3u ? c3 : result; result = clog == 2u ? c2 : result;
    result = clog == 1u ? c1 : result;
    if (lane == 0u) __hip_atomic_store(tickets + (size_t)w.voice * TICKET_STRIDE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
}

// A program's load.  `input(row)` is S_INPUT: the block's one row, or a republished control row.  An input with a history (the
// hist form's StreamHistInput; kernels.hpp bank_stream_hist_kernel has the argument) also serves S_READ_INPUT: the streamed row
// imm, d_lo frames back, 0.0 before frame 0 -- a frame-only load like the others, so it goes out with a program's leading loads.
template <class Input>
constexpr bool stream_has_history = std::remove_reference_t<Input>::history;
template <class Input>
__device__ __forceinline__ float stream_prog_load(const StreamProgArgs &p, const StageInstr &in, uint64_t frame, Input &&input) {
    switch (in.op) {
    case S_CONST: return __uint_as_float(in.imm);
    case S_INPUT: return input(in.imm);
    case S_READ:
        return frame >= in.d_lo ? __hip_atomic_load(p.rings + (size_t)in.buf * (p.ring_mask + 1) + ((frame - in.d_lo) & p.ring_mask), __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT)
                                : 0.0f;
    case S_READ_INPUT:
        if constexpr (stream_has_history<Input>) return frame >= in.d_lo ? input.at(in.imm, frame - in.d_lo) : 0.0f;
        [[fallthrough]];
    default: return frame >= in.d_lo ? __uint_as_float(in.imm) : 0.0f;   // S_STEP
    }
}

// A Delay by a signal amount (FR_STREAM_DYN; kernels.hpp bank_stream_dyn_kernel), lane = frame: the reference's cast of the
// amount (delay_frames, as pull_kernel and stage_kernel), then S_READ_DYN reads the ring `frames` back and S_STEP_DYN yields its
// constant; 0.0 where the cast fails or the source frame lies before frame 0.  The rule admits a bank's ring and (FR_STREAM_TAPS)
// a ring that an EARLIER program of the same voice, segment or bus segment stores: this wave (a bus program: every voice and every
// voice's programs) has stored and acknowledged the block's frames -- stream_run_programs waits for its own stores before every
// program --, earlier blocks everything older, so the load -- L2's, never a CU's L1: the finisher of a voice changes CU from block
// to block -- finds any offset in [0, bound].  The index is masked.
__device__ __forceinline__ float stream_prog_dyn(const float *rings, uint64_t ring_mask, uint32_t sparkle, uint32_t op, uint32_t imm, uint32_t buf, float amount,
                                                 uint64_t frame) {
    uint64_t fr;
    if (!delay_frames(amount, fr, sparkle != 0u) || frame < fr) return 0.0f;
    if (op == S_STEP_DYN) return __uint_as_float(imm);
    return __hip_atomic_load(rings + (size_t)buf * (ring_mask + 1) + ((frame - fr) & ring_mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The interpreter: programs [p_first, p_end) in order, lane = frame, in wave 0 of a finishing workgroup; `regs` are its
// registers, [register][lane] in LDS; `out` the mapped host rows.  DYN: it also knows S_READ_DYN and S_STEP_DYN; with an input that
// has a history (stream_has_history) S_READ_INPUT_DYN too: stream_prog_dyn with the history as its rings and the streamed row as
// the ring -- the same cast, the same range test, the same masked relaxed agent-scope load.
template <bool DYN = false, class Input>
__device__ __forceinline__ void stream_run_programs(float *out, const StreamProgArgs &p, float (&regs)[STAGE_REGS][64], uint32_t p_first, uint32_t p_end, uint64_t frame,
                                                    uint32_t lane, bool live, Input &&input) {
    const uint64_t ring_cap = p.ring_mask + 1;
    for (uint32_t pi = p_first; pi < p_end; ++pi) {
        // what this wave has stored so far (the voice's ring, an earlier program's rings) is in L2 before it is read back
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const StageProg pg = p.progs[pi];
        const StageInstr *ins = p.instrs + pg.first_instr;
        uint32_t i = 0;
        for (; i + 4u <= pg.n_loads; i += 4u) {   // the program's leading loads (rings and control rows), four round trips to L2 in flight together
            float ld[4];
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) ld[j] = stream_prog_load(p, ins[i + j], frame, input);
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) regs[ins[i + j].dst][lane] = ld[j];
        }
        for (; i < pg.n_instr; ++i) {
            const StageInstr in = ins[i];
            float v;
            switch (in.op) {
            STAGE_ARITH_CASES(v, regs[in.a][lane], regs[in.b][lane], p.sparkle != 0u)
            case S_STORE:
                if (live) __hip_atomic_store(p.rings + (size_t)in.buf * ring_cap + (frame & p.ring_mask), regs[in.a][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                continue;
            case S_READ_DYN: case S_STEP_DYN:
                if constexpr (DYN) {
                    v = stream_prog_dyn(p.rings, p.ring_mask, p.sparkle, in.op, in.imm, in.buf, regs[in.a][lane], frame);
                    break;
                }
                [[fallthrough]];
            case S_READ_INPUT_DYN:
                if constexpr (DYN && stream_has_history<Input>) {
                    v = stream_prog_dyn(input.hist, input.hmask, p.sparkle, S_READ_DYN, 0u, in.imm & (BANK_STREAM_ROWS - 1u), regs[in.a][lane], frame);
                    break;
                }
                [[fallthrough]];
            default: v = stream_prog_load(p, in, frame, input); break;
            }
            regs[in.dst][lane] = v;
        }
        const float res = regs[pg.result_reg][lane];
        if (live && pg.dst_ring != 0xFFFFFFFFu)
            __hip_atomic_store(p.rings + (size_t)pg.dst_ring * ring_cap + (frame & p.ring_mask), res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (live && pg.out_row >= 0) __hip_atomic_store(out + (size_t)pg.out_row * 64u + lane, res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// A loop program (FR_STREAM_LOOPS; kernels.hpp bank_stream_loops_kernel): StageProg::pad[0] = its stride, 1..63.  The block's
// n frames start at `head`; `ldt` and `stt` are the load and the store tile.  One wave runs this, so the phases are ordered by
// the wave's own program order (LDS accesses of a wave complete in order); the wavefront-scope fences keep the compiler from
// moving an access across a phase boundary and emit nothing.
__device__ __forceinline__ void stream_wave_phase() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// Instruction i of a loop program: from the wave's LDS copy of its first BANK_STREAM_LOOP_INSTRS instructions (phase 2 fetches
// every instruction once per FRAME: from global memory that is a dependent trip to L2 each), the rest from memory.  Uniform: the
// words go to scalar registers.
__device__ __forceinline__ StageInstr stream_loop_instr(const uint4 (&lins)[BANK_STREAM_LOOP_INSTRS], const StageInstr *ins, uint32_t i) {
    uint4 w = i < BANK_STREAM_LOOP_INSTRS ? lins[i] : *reinterpret_cast<const uint4 *>(ins + i);
    w.x = __builtin_amdgcn_readfirstlane(w.x);
    w.y = __builtin_amdgcn_readfirstlane(w.y);
    w.z = __builtin_amdgcn_readfirstlane(w.z);
    w.w = __builtin_amdgcn_readfirstlane(w.w);
    StageInstr in;
    static_assert(sizeof(StageInstr) == sizeof(uint4), "an instruction is four words");
    __builtin_memcpy(&in, &w, sizeof in);
    return in;
}

// SWEEP (FR_STREAM_SWEEP; kernels.hpp bank_stream_sweep_kernel, where the argument stands): pad[0] is the program's sweep width w
// (a loop program of constant stride: its stride), and phase 2 walks the block w frames at a time, lanes < w a frame each, with
// the Delays by a signal amount among its cases.  Phases 0, 1 and 3 are the same.
template <bool SWEEP = false, class Input>
__device__ __forceinline__ void stream_run_loop_program(float *out, const StreamProgArgs &p, float (&regs)[STAGE_REGS][64], float (&ldt)[BANK_STREAM_LOOP_LOADS][64],
                                                        float (&stt)[BANK_STREAM_LOOP_STORES][64], uint4 (&lins)[BANK_STREAM_LOOP_INSTRS], const StageProg &pg, uint64_t head,
                                                        uint32_t n, uint32_t lane, bool live, Input &&input) {
    constexpr uint32_t LM = BANK_STREAM_LOOP_LOADS - 1u, SM = BANK_STREAM_LOOP_STORES - 1u;
    const uint64_t ring_cap = p.ring_mask + 1;
    const uint64_t frame = head + lane;
    const StageInstr *ins = p.instrs + pg.first_instr;
    const uint32_t stride = pg.pad[0] < BANK_STREAM_LOOP_MAX_STRIDE ? pg.pad[0] : BANK_STREAM_LOOP_MAX_STRIDE;
    n = n < 64u ? n : 64u;
    // 0. the program's instructions to LDS, a lane each
    for (uint32_t i = lane; i < pg.n_instr && i < BANK_STREAM_LOOP_INSTRS; i += 64u) lins[i] = *reinterpret_cast<const uint4 *>(ins + i);
    stream_wave_phase();
    auto fetch = [&](uint32_t i) { return stream_loop_instr(lins, ins, i); };
    // 1. the loads that depend on the frame alone, lane = frame: four round trips to L2 in flight together
    {
        uint32_t k = 0;
        for (uint32_t i = 0; i < pg.n_instr;) {
            uint32_t at0 = 0, at1 = 0, at2 = 0, at3 = 0, m = 0;   // the next (up to) four loads: the last m of at0..at3
            for (; i < pg.n_instr && m < 4u; ++i) {
                const uint32_t op = fetch(i).op;
                if (op == S_INPUT || op == S_READ || (stream_has_history<Input> && op == S_READ_INPUT)) { at0 = at1; at1 = at2; at2 = at3; at3 = i; ++m; }
            }
            const uint32_t at[4] = {at0, at1, at2, at3};
            float ld[4];
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                ld[j] = 0.0f;
                if (j + m >= 4u) {
                    const StageInstr in = fetch(at[j]);
                    const bool inside = in.op == S_READ && in.imm != 0u && lane >= in.d_lo;   // phase 2 takes it from the store tile
                    if (live && !inside) ld[j] = stream_prog_load(p, in, frame, input);
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j)
                if (j + m >= 4u) ldt[(k + j + m - 4u) & LM][lane] = ld[j];
            k += m;
        }
    }
    stream_wave_phase();
    // 2. (SWEEP) the sweeps: frames [base, base + w) read store-tile columns below `base` only, which earlier iterations of this
    // wave wrote; the loop's bounds are uniform for the wave, and every sweep ends in a wave phase
    if constexpr (SWEEP) {
        const uint32_t w = stride != 0u ? stride : 1u;
        for (uint32_t base = 0; base < n; base += w) {
            const uint32_t f = base + lane;
            if (lane < w && f < n) {
                uint32_t k = 0;
                for (uint32_t i = 0; i < pg.n_instr; ++i) {
                    const StageInstr in = fetch(i);
                    float v;
                    switch (in.op) {
                    case S_CONST: v = __uint_as_float(in.imm); break;
                    case S_STEP: v = head + f >= in.d_lo ? __uint_as_float(in.imm) : 0.0f; break;
                    case S_INPUT: v = ldt[k++ & LM][f]; break;
                    case S_READ: {
                        const uint32_t slot = k++ & LM;
                        v = in.imm != 0u && f >= in.d_lo ? stt[(in.imm - 1u) & SM][(f - in.d_lo) & 63u] : ldt[slot][f];
                        break;
                    }
                    STAGE_ARITH_CASES(v, regs[in.a][f], regs[in.b][f], p.sparkle != 0u)
                    case S_STORE: stt[(in.imm - 1u) & SM][f] = regs[in.a][f]; continue;
                    case S_READ_DYN: {
                        // an own ring (imm = store slot + 1) at a frame of this block: the store tile; else the masked load
                        uint64_t fr;
                        if (!delay_frames(regs[in.a][f], fr, p.sparkle != 0u) || head + f < fr) v = 0.0f;
                        else if (in.imm != 0u && fr <= f) v = stt[(in.imm - 1u) & SM][(f - (uint32_t)fr) & 63u];
                        else v = __hip_atomic_load(p.rings + (size_t)in.buf * ring_cap + ((head + f - fr) & p.ring_mask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                    case S_STEP_DYN: v = stream_prog_dyn(p.rings, p.ring_mask, p.sparkle, S_STEP_DYN, in.imm, in.buf, regs[in.a][f], head + f); break;
                    case S_READ_INPUT_DYN:
                        if constexpr (stream_has_history<Input>) {
                            v = stream_prog_dyn(input.hist, input.hmask, p.sparkle, S_READ_DYN, 0u, in.imm & (BANK_STREAM_ROWS - 1u), regs[in.a][f], head + f);
                            break;
                        }
                        [[fallthrough]];
                    case S_READ_INPUT:          // (an input with a history: phase 1 loaded it like an S_INPUT)
                        if constexpr (stream_has_history<Input>) {
                            v = ldt[k++ & LM][f];
                            break;
                        }
                        [[fallthrough]];
                    default: v = 0.0f; break;
                    }
                    regs[in.dst][f] = v;
                }
            }
            stream_wave_phase();
        }
    } else
    // 2. the loops, a lane per residue, every frame on its own register column
    if (lane < stride) {
        for (uint32_t f = lane; f < n; f += stride) {
            uint32_t k = 0;
            for (uint32_t i = 0; i < pg.n_instr; ++i) {
                const StageInstr in = fetch(i);
                float v;
                switch (in.op) {
                case S_CONST: v = __uint_as_float(in.imm); break;
                case S_STEP: v = head + f >= in.d_lo ? __uint_as_float(in.imm) : 0.0f; break;
                case S_INPUT: v = ldt[k++ & LM][f]; break;
                case S_READ: {
                    const uint32_t slot = k++ & LM;
                    v = in.imm != 0u && f >= in.d_lo ? stt[(in.imm - 1u) & SM][(f - in.d_lo) & 63u] : ldt[slot][f];
                    break;
                }
                STAGE_ARITH_CASES(v, regs[in.a][f], regs[in.b][f], p.sparkle != 0u)
                case S_STORE: stt[(in.imm - 1u) & SM][f] = regs[in.a][f]; continue;
                case S_READ_INPUT:          // (an input with a history: phase 1 loaded it like an S_INPUT)
                    if constexpr (stream_has_history<Input>) {
                        v = ldt[k++ & LM][f];
                        break;
                    }
                    [[fallthrough]];
                default: v = 0.0f; break;   // (a Delay of a signal amount; without a history a delayed input: the rule serves no such program)
                }
                regs[in.dst][f] = v;
            }
        }
    }
    stream_wave_phase();
    // 3. the block's stores, lane = frame
    for (uint32_t i = 0; i < pg.n_instr; ++i) {
        const StageInstr in = fetch(i);
        if (in.op == S_STORE && live)
            __hip_atomic_store(p.rings + (size_t)in.buf * ring_cap + (frame & p.ring_mask), stt[(in.imm - 1u) & SM][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const float res = regs[pg.result_reg][lane];
    if (live && pg.dst_ring != 0xFFFFFFFFu)
        __hip_atomic_store(p.rings + (size_t)pg.dst_ring * ring_cap + (frame & p.ring_mask), res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (live && pg.out_row >= 0) __hip_atomic_store(out + (size_t)pg.out_row * 64u + lane, res, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    stream_wave_phase();   // (the next program's phases write the tiles this one has read)
}

// stream_run_programs where a program may be a loop program; one of stride 0 is a range of one program of stream_run_programs.
// (DYN concerns those alone: without SWEEP the rule serves no loop program with a Delay by a signal amount.)
template <bool DYN = false, bool SWEEP = false, class Input>
__device__ __forceinline__ void stream_run_programs_loops(float *out, const StreamProgArgs &p, float (&regs)[STAGE_REGS][64], float (&ldt)[BANK_STREAM_LOOP_LOADS][64],
                                                          float (&stt)[BANK_STREAM_LOOP_STORES][64], uint4 (&lins)[BANK_STREAM_LOOP_INSTRS], uint32_t p_first,
                                                          uint32_t p_end, uint64_t head, uint32_t n, uint32_t lane, bool live, Input &&input) {
    for (uint32_t pi = p_first; pi < p_end; ++pi) {
        if (p.progs[pi].pad[0] == 0u) {
            stream_run_programs<DYN>(out, p, regs, pi, pi + 1u, head + lane, lane, live, input);
            continue;
        }
        // what this wave has stored so far (the voice's ring, an earlier program's rings) is in L2 before it is read back
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const StageProg pg = p.progs[pi];
        if constexpr (SWEEP) stream_run_loop_program<true>(out, p, regs, ldt, stt, lins, pg, head, n, lane, live, input);
        else stream_run_loop_program(out, p, regs, ldt, stt, lins, pg, head, n, lane, live, input);
    }
}

// A finished voice's frames, head + lane, go to its ring or -- a host row: system scope -- to its row, as its bank says.
__device__ __forceinline__ void stream_store_voice(const StreamWork &w, float *out, const StreamProgArgs &p, uint64_t frame, uint32_t lane, bool live, float result) {
    const uint32_t dst = w.rows[w.bank_voice];
    if (live) {
        if (w.to_ring) __hip_atomic_store(p.rings + (size_t)dst * (p.ring_mask + 1) + (frame & p.ring_mask), result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else __hip_atomic_store(out + (size_t)dst * 64u + lane, result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The finishing wave counts its voice in.  Ring and row stores alike are acknowledged before the ticket, so the block's done
// tag -- written by the lane that counts the last voice in -- implies that every store of the block has landed.
template <class Ctl, class Dev>
__device__ __forceinline__ void stream_finish(Ctl *ctl, Dev *dev, uint32_t n_voices, uint32_t lane, uint32_t seq) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0u) {
        const uint32_t n = __hip_atomic_fetch_add(&dev->voices_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n == n_voices - 1u) {
            __hip_atomic_store(&dev->voices_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&ctl->done, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// The same with a bus segment: the ticket goes to the whole wave, and the block's last arriver runs `bus` (the programs that
// read several voices of this block), lane = frame, before the tag.  Every voice's stores were acknowledged before its ticket,
// and this wave's loads are issued after its own ticket came back: the hand-over of the chunk sums.
template <class Ctl, class Dev, class Bus>
__device__ __forceinline__ void stream_finish_bus(Ctl *ctl, Dev *dev, uint32_t n_voices, uint32_t lane, uint32_t seq, Bus &&bus) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t n = 0u;
    if (lane == 0u) n = __hip_atomic_fetch_add(&dev->voices_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    n = __builtin_amdgcn_readfirstlane(n);
    if (n == n_voices - 1u) {
        bus();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // host rows and rings have landed before the done tag
        if (lane == 0u) {
            __hip_atomic_store(&dev->voices_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&ctl->done, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// Workgroups launch_bank uses for this shape.
uint64_t bank_blocks(const BankArgs &a) {
    uint64_t f = a.frames_per_lane;
    return ((a.n_times + 64 * f - 1) / (64 * f)) * a.n_voices << (a.log2_p - a.chunk_log2);
}

template <int F>
static hipError_t launch_bank_f(const BankArgs &a, hipStream_t s) {
    uint64_t nblocks64 = bank_blocks(a);
    if (nblocks64 == 0) return hipSuccess;
    if (nblocks64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    uint32_t tiles = (uint32_t)((a.n_times + 64 * F - 1) / (64 * F)), nblocks = (uint32_t)nblocks64;
    const bool w8 = a.waves_per_group == 8;
    if (a.leaf_variant == 0) {
        if (w8) hipLaunchKernelGGL((bank_kernel<F, 0, 8>), dim3(nblocks), dim3(512), 0, s, a, tiles, nblocks);
        else hipLaunchKernelGGL((bank_kernel<F, 0, 4>), dim3(nblocks), dim3(256), 0, s, a, tiles, nblocks);
    } else if (a.leaf_variant == 1 && a.host_flags && a.chunk_log2 == a.log2_p) {   // (bank_publishes_rows)
        if (w8) hipLaunchKernelGGL((bank_kernel<F, 1, 8, true>), dim3(nblocks), dim3(512), 0, s, a, tiles, nblocks);
        else hipLaunchKernelGGL((bank_kernel<F, 1, 4, true>), dim3(nblocks), dim3(256), 0, s, a, tiles, nblocks);
    } else if (a.leaf_variant == 1) {
        if (w8) hipLaunchKernelGGL((bank_kernel<F, 1, 8>), dim3(nblocks), dim3(512), 0, s, a, tiles, nblocks);
        else if (a.waves_per_group == 2 && a.chunk_log2 <= 12) hipLaunchKernelGGL((bank_kernel<F, 1, 2>), dim3(nblocks), dim3(128), 0, s, a, tiles, nblocks);
        else if (a.waves_per_group == 1 && a.chunk_log2 <= 11) hipLaunchKernelGGL((bank_kernel<F, 1, 1>), dim3(nblocks), dim3(64), 0, s, a, tiles, nblocks);
        else hipLaunchKernelGGL((bank_kernel<F, 1, 4>), dim3(nblocks), dim3(256), 0, s, a, tiles, nblocks);
    } else {
        hipLaunchKernelGGL((bank_kernel<F, 2, 4>), dim3(nblocks), dim3(256), 0, s, a, tiles, nblocks);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || a.chunk_log2 == a.log2_p) return e;
    uint64_t total = (uint64_t)a.n_voices * a.n_times;
    hipLaunchKernelGGL(bank_combine_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_bank(const BankArgs &a, hipStream_t s) {
    if (a.small_call == 2) {   // short calls: chunks over workgroups, LDS-staged parameters, in-launch combine
        if (a.chunk_log2 < 7 || a.chunk_log2 > 13 || a.chunk_log2 > a.log2_p || a.log2_p - a.chunk_log2 > 8) return hipErrorInvalidValue;
        if (a.chunk_log2 != a.log2_p && (!a.ws || !a.tickets)) return hipErrorInvalidValue;
        if ((8u << a.chunk_log2) / (8u * a.waves_per_group) < 8u) return hipErrorInvalidValue;   // a wave needs a whole group
        switch (a.waves_per_group) {
        case 4: return launch_bank_short<4>(a, s);
        case 8: return launch_bank_short<8>(a, s);
        case 16: return launch_bank_short<16>(a, s);
        default: return hipErrorInvalidValue;
        }
    }
    if (a.small_call) {   // lanes over partials
        if (a.log2_p < 8 || a.log2_p > 24 || a.n_times > SMALL_MAX_FRAMES || a.chunk_log2 != 8) return hipErrorInvalidValue;
        if (a.log2_p != 8 && !a.ws) return hipErrorInvalidValue;
        if (a.n_times == 0 || a.n_voices == 0) return hipSuccess;
        if (a.n_voices > 65535u) return hipErrorInvalidValue;
        hipLaunchKernelGGL(bank_small_kernel, dim3(1u << (a.log2_p - 8u), a.n_voices), dim3(256), 0, s, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess || a.log2_p == 8) return e;
        uint64_t total = (uint64_t)a.n_voices * a.n_times;
        hipLaunchKernelGGL(bank_combine_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if (a.voices_per_wave) {   // many small voices: whole voices per wave
        if (a.log2_p < 3 || a.log2_p > 8 || a.chunk_log2 != a.log2_p || a.voices_per_wave > 64) return hipErrorInvalidValue;
        if (a.n_times == 0 || a.n_voices == 0) return hipSuccess;
        const uint32_t F = a.frames_per_lane;
        if (F != 1 && F != 2) return hipErrorInvalidValue;
        const uint64_t tiles = (a.n_times + 64 * F - 1) / (64 * F);
        const uint64_t vgroups = ((uint64_t)a.n_voices + 4ull * a.voices_per_wave - 1) / (4ull * a.voices_per_wave);
        const uint64_t nb = tiles * vgroups;
        if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
        const int mode = a.leaf_variant > 2 ? 1 : (int)a.leaf_variant;
        if (F == 1) {
            if (mode == 0) hipLaunchKernelGGL((bank_multi_kernel<1, 0>), dim3((uint32_t)nb), dim3(256), 0, s, a, (uint32_t)tiles, (uint32_t)nb);
            else if (mode == 1) hipLaunchKernelGGL((bank_multi_kernel<1, 1>), dim3((uint32_t)nb), dim3(256), 0, s, a, (uint32_t)tiles, (uint32_t)nb);
            else hipLaunchKernelGGL((bank_multi_kernel<1, 2>), dim3((uint32_t)nb), dim3(256), 0, s, a, (uint32_t)tiles, (uint32_t)nb);
        } else {
            if (mode == 0) hipLaunchKernelGGL((bank_multi_kernel<2, 0>), dim3((uint32_t)nb), dim3(256), 0, s, a, (uint32_t)tiles, (uint32_t)nb);
            else if (mode == 1) hipLaunchKernelGGL((bank_multi_kernel<2, 1>), dim3((uint32_t)nb), dim3(256), 0, s, a, (uint32_t)tiles, (uint32_t)nb);
            else hipLaunchKernelGGL((bank_multi_kernel<2, 2>), dim3((uint32_t)nb), dim3(256), 0, s, a, (uint32_t)tiles, (uint32_t)nb);
        }
        return hipGetLastError();
    }
    if (a.waves_per_group != 4 && a.waves_per_group != 8 && a.waves_per_group != 2 && a.waves_per_group != 1) return hipErrorInvalidValue;
    if (a.waves_per_group < 4 && (a.leaf_variant != 1 || a.host_flags)) return hipErrorInvalidValue;   // (1- and 2-wave workgroups: FMA-form leaves only)
    // a wave sums 8 .. 2048 partials (whole groups of 8, at most 8 carry levels)
    const uint32_t cmin = a.waves_per_group == 8 ? 6 : a.waves_per_group == 4 ? 5 : a.waves_per_group == 2 ? 4 : 3;
    const uint32_t cmax = a.waves_per_group == 8 ? 14 : a.waves_per_group == 4 ? 13 : a.waves_per_group == 2 ? 12 : 11;
    if (a.log2_p < cmin || a.log2_p > 24 || a.chunk_log2 < cmin || a.chunk_log2 > cmax || a.chunk_log2 > a.log2_p)
        return hipErrorInvalidValue;
    if (a.chunk_log2 != a.log2_p && !a.ws) return hipErrorInvalidValue;
    switch (a.frames_per_lane) {
    case 1: return launch_bank_f<1>(a, s);
    case 2: return launch_bank_f<2>(a, s);
    case 4: return launch_bank_f<4>(a, s);
    default: return hipErrorInvalidValue;
    }
}

// ---------------------------------------------------------------------------------------------------
// General voices: the same leaf, any Sum2 tree (odd carries, unbalanced, non-power-of-two partial counts).
// The host cuts the tree into items = maximal complete sub-trees of up to 2048 consecutive leaves and a post-order
// schedule "item, then m merges"; one workgroup per (voice, 64-frame tile) runs it (gbank_tile below).  Same bits as
// the graph: every add is the tree's own add.
// ---------------------------------------------------------------------------------------------------
// The evaluation stack lives in LDS as [level][lane] columns (a lane only touches its own column: no barriers, no
// bank conflicts); its pointer is wave-uniform.  (A first version kept the stack in 16 named registers selected by
// compare ladders: 32 v_cndmask per group, 4x slower than the balanced kernel; profiles/r01_general_tree.txt.)
constexpr uint32_t GB_MAX_DEPTH = 16;

template <bool FAST>
__device__ __forceinline__ float gbank_group(const ParamGroup &pg, uint32_t j, float t) {
    float l0 = bank_leaf<FAST, false>(t, pg.w[0], pg.A[0]);
    float v = l0;
    if (j >= 1u) {
        float l1 = bank_leaf<FAST, false>(t, pg.w[1], pg.A[1]);
        v = l0 + l1;
        if (j >= 2u) {
            float l2 = bank_leaf<FAST, false>(t, pg.w[2], pg.A[2]);
            float l3 = bank_leaf<FAST, false>(t, pg.w[3], pg.A[3]);
            v = v + (l2 + l3);
            if (j >= 3u) {
                float l4 = bank_leaf<FAST, false>(t, pg.w[4], pg.A[4]);
                float l5 = bank_leaf<FAST, false>(t, pg.w[5], pg.A[5]);
                float l6 = bank_leaf<FAST, false>(t, pg.w[6], pg.A[6]);
                float l7 = bank_leaf<FAST, false>(t, pg.w[7], pg.A[7]);
                v = v + ((l4 + l5) + (l6 + l7));
            }
        }
    }
    return v;
}

// One workgroup (4 waves) per (voice, 64-frame tile).  Items of >= 32 leaves are complete sub-trees: each wave sums a
// quarter of the item with the balanced kernel's inner loop (parameters through the scalar cache, register carry
// chain), the four quarter sums meet in LDS in the tree's own association; smaller items are evaluated by wave 0
// alone.  Wave 0 then runs the merge schedule on its LDS stack.  One barrier per big item (double-buffered hand-over:
// item i+2 reuses item i's buffer only after the barrier of item i+1, which wave 0 reaches after reading item i's).
template <bool FAST>
__device__ __forceinline__ float gbank_tile(const float *params, const uint32_t *gmeta, uint32_t nitems, float t, uint32_t wave, uint32_t lane,
                                            float *stack /* wave 0: [GB_MAX_DEPTH][64] + lane */, float (*sm)[64]) {
    uint32_t sp = 0;
    const_f32_ptr p = (const_f32_ptr)params;
    typedef uint32_t __attribute__((address_space(4))) const *const_u32_ptr;
    const_u32_ptr gm = (const_u32_ptr)gmeta;
    auto finish = [&](float v, uint32_t meta) {        // wave 0 only
        for (uint32_t m = meta >> 4; m != 0u; --m) {   // v = pop() + v
            --sp;
            v = stack[sp * 64u] + v;
        }
        stack[sp * 64u] = v;
        ++sp;
    };
    uint32_t goff = 0;          // parameter group (8 pairs) the current item starts at
    uint32_t nbig = 0;
    for (uint32_t i = 0; i < nitems; ++i) {
        const uint32_t meta = gm[i];
        const uint32_t k = meta & 15u;
        const float tt[1] = {t};
        float res[1];
        if (k >= 5u) {          // 32..2048 leaves: a quarter (2^(k-5) groups of 8) per wave
            const uint32_t gq = 1u << (k - 5u);
            bank_wave_sum<1, FAST, false>(params + ((size_t)goff + (size_t)wave * gq) * 16u, gq, k - 5u, tt, res);
            float(*buf)[64] = sm + 4u * (nbig & 1u);   // double-buffered: the next item's sums do not wait for wave 0 to read these
            ++nbig;
            buf[wave][lane] = res[0];
            __syncthreads();
            if (wave == 0u) finish((buf[0][lane] + buf[1][lane]) + (buf[2][lane] + buf[3][lane]), meta);
            goff += 1u << (k - 3u);
        } else if (wave == 0u) {
            if (k == 4u) {      // 16 leaves: two groups
                bank_wave_sum<1, FAST, false>(params + (size_t)goff * 16u, 2u, 1u, tt, res);
                finish(res[0], meta);
            } else {
                ParamGroup cur;
                load_group(cur, p, goff);
                __builtin_amdgcn_s_waitcnt(0xC07F);
                finish(gbank_group<FAST>(cur, k, t), meta);
            }
            goff += k == 4u ? 2u : 1u;
        } else {
            goff += k == 4u ? 2u : 1u;
        }
    }
    return wave == 0u ? stack[0] : 0.0f;   // a well-formed schedule leaves exactly the root
}

__global__ void __launch_bounds__(256) gbank_kernel(BankArgs a, uint32_t tiles, uint32_t nblocks) {
    __shared__ float stack_mem[GB_MAX_DEPTH][64];
    __shared__ float sm[8][64];
    uint32_t b = blockIdx.x;
    uint32_t lid = (nblocks % 8u == 0u) ? (b % 8u) * (nblocks / 8u) + b / 8u : b;
    const uint32_t voice = lid / tiles;
    const uint32_t tile = lid - voice * tiles;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t ti = (uint64_t)tile * 64u + lane;
    const float t = bank_time(a, ti);
    const bool fast = a.fast_ok && __all(t >= 0.0f && t <= 4294967296.0f);   // same for the 4 waves: same 64 frames
    const uint32_t i0 = a.group_off[2u * voice], ni = a.group_off[2u * voice + 2u] - i0;
    const float2 *vparams = a.params + (size_t)a.group_off[2u * voice + 1u] * 8u;
    float *stack = &stack_mem[0][lane];
    float r = fast ? gbank_tile<true>((const float *)vparams, a.groups + i0, ni, t, wave, lane, stack, sm)
                   : gbank_tile<false>((const float *)vparams, a.groups + i0, ni, t, wave, lane, stack, sm);
    float *orow = a.out + (size_t)a.rows[voice] * a.out_stride;
    const bool live = ti < a.n_times;
    if (wave == 0u && live) orow[bank_out_index(a, ti)] = r;
    // sign of a zero result: -0 iff every (valid) leaf is -0, see leaves_all_negzero
    __shared__ unsigned long long zshared;
    if (wave == 0u) {
        unsigned long long z = __ballot(live && r == 0.0f);
        if (lane == 0u) zshared = z;
    }
    __syncthreads();
    unsigned long long zm = zshared;   // workgroup-uniform
    if (zm == 0ull) return;
    if (__builtin_popcountll(zm) > 4) {
        // many zero frames (a silent voice): all 64 frames at once, items of >= 32 leaves split over the 4 waves like
        // the sums were, the few leaves of smaller items on wave 0 (padding pairs are not leaves and are skipped)
        bool ok = true;
        uint32_t goff = 0;
        const float *fp = (const float *)vparams;
        for (uint32_t i = 0; i < ni; ++i) {
            const uint32_t kk = a.groups[i0 + i] & 15u;
            if (kk >= 5u) {
                const uint32_t gq = 1u << (kk - 5u);
                const float *q = fp + ((size_t)goff + (size_t)wave * gq) * 16u;
                ok = ok && (fast ? wave_leaves_all_negzero<true>(q, gq, t, zm) : wave_leaves_all_negzero<false>(q, gq, t, zm));
                goff += 1u << (kk - 3u);
            } else {
                if (wave == 0u) {
                    const uint32_t sz = 1u << kk;
                    for (uint32_t j = 0; j < sz; ++j) {
                        const float2 pr = vparams[(size_t)goff * 8u + j];   // wave-uniform address
                        const float lf = fast ? bank_leaf<true, true>(t, pr.x, pr.y) : bank_leaf<false, true>(t, pr.x, pr.y);
                        ok = ok && __float_as_uint(lf) == 0x80000000u;
                    }
                }
                goff += kk == 4u ? 2u : 1u;
            }
        }
        sm[wave][lane] = ok ? 1.0f : 0.0f;     // (every wave is past the last hand-over of gbank_tile: zshared's barrier)
        __syncthreads();
        if (wave == 0u && ((zm >> lane) & 1ull)) {
            const bool all = sm[0][lane] != 0.0f && sm[1][lane] != 0.0f && sm[2][lane] != 0.0f && sm[3][lane] != 0.0f;
            orow[bank_out_index(a, ti)] = all ? -0.0f : 0.0f;
        }
        return;
    }
    if (wave != 0u) return;
    while (zm) {
        uint32_t l = (uint32_t)__builtin_ctzll(zm);
        zm &= zm - 1;
        uint64_t tz_i = (uint64_t)tile * 64u + l;
        float tz = bank_time(a, tz_i);
        bool ok = true;
        uint32_t pair0 = 0;   // first parameter pair of the item
        for (uint32_t i = 0; i < ni && ok; ++i) {
            const uint32_t kk = a.groups[i0 + i] & 15u, sz = 1u << kk;
            for (uint32_t q = lane; q < sz && ok; q += 64u) {
                float2 p = vparams[pair0 + q];
                ok = __float_as_uint(bank_leaf<false, true>(tz, p.x, p.y)) == 0x80000000u;
            }
            ok = __all(ok);
            pair0 += sz < 8u ? 8u : sz;
        }
        if (lane == 0) orow[bank_out_index(a, tz_i)] = ok ? -0.0f : 0.0f;
    }
}

// Many small general voices: like bank_multi_kernel, a wave runs WHOLE voices (items + merge schedule), several in a
// row, for one 64-frame tile; each wave has its own LDS stack; no barriers.
template <bool FAST>
__device__ __forceinline__ float gbank_voice(const float *params, const uint32_t *gmeta, uint32_t nitems, float t, float *stack /* [GB_MAX_DEPTH][64] + lane */) {
    uint32_t sp = 0;
    const_f32_ptr p = (const_f32_ptr)params;
    typedef uint32_t __attribute__((address_space(4))) const *const_u32_ptr;
    const_u32_ptr gm = (const_u32_ptr)gmeta;
    auto finish = [&](float v, uint32_t meta) {
        for (uint32_t m = meta >> 4; m != 0u; --m) {   // v = pop() + v
            --sp;
            v = stack[sp * 64u] + v;
        }
        stack[sp * 64u] = v;
        ++sp;
    };
    uint32_t goff = 0;
    for (uint32_t i = 0; i < nitems; ++i) {
        const uint32_t meta = gm[i];
        const uint32_t k = meta & 15u;
        if (k > 3u) {
            const float tt[1] = {t};
            float res[1];
            bank_wave_sum<1, FAST, false>(params + (size_t)goff * 16u, 1u << (k - 3u), k - 3u, tt, res);
            finish(res[0], meta);
            goff += 1u << (k - 3u);
        } else {
            ParamGroup cur;
            load_group(cur, p, goff);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            finish(gbank_group<FAST>(cur, k, t), meta);
            goff += 1u;
        }
    }
    return stack[0];
}

__global__ void __launch_bounds__(256) gbank_multi_kernel(BankArgs a, uint32_t tiles, uint32_t nblocks) {
    __shared__ float stack_mem[4][GB_MAX_DEPTH][64];
    uint32_t b = blockIdx.x;
    uint32_t lid = (nblocks % 8u == 0u) ? (b % 8u) * (nblocks / 8u) + b / 8u : b;
    const uint32_t vb = lid / tiles, tile = lid - vb * tiles;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t ti = (uint64_t)tile * 64u + lane;
    const float t = bank_time(a, ti);
    const bool fast = a.fast_ok && __all(t >= 0.0f && t <= 4294967296.0f);
    const bool live = ti < a.n_times;
    float *stack = &stack_mem[wave][0][lane];
    const uint32_t v0 = (vb * 4u + wave) * a.voices_per_wave;
    for (uint32_t j = 0; j < a.voices_per_wave; ++j) {
        const uint32_t voice = v0 + j;
        if (voice >= a.n_voices) break;                      // wave-uniform
        const uint32_t i0 = a.group_off[2u * voice], ni = a.group_off[2u * voice + 2u] - i0;
        const float2 *vparams = a.params + (size_t)a.group_off[2u * voice + 1u] * 8u;
        const float r = fast ? gbank_voice<true>((const float *)vparams, a.groups + i0, ni, t, stack)
                             : gbank_voice<false>((const float *)vparams, a.groups + i0, ni, t, stack);
        float *orow = a.out + (size_t)a.rows[voice] * a.out_stride;
        if (live) orow[bank_out_index(a, ti)] = r;
        // sign of exact zeros (see leaves_all_negzero), within the wave
        unsigned long long zm = __ballot(live && r == 0.0f);
        if (zm == 0ull) continue;
        if (__builtin_popcountll(zm) > 4) {                  // a silent voice: all 64 frames in one pass over its items
            bool ok = true;
            uint32_t goff = 0;
            for (uint32_t i = 0; i < ni; ++i) {
                const uint32_t kk = a.groups[i0 + i] & 15u;
                if (kk > 3u) {
                    const float *q = (const float *)vparams + (size_t)goff * 16u;
                    ok = ok && (fast ? wave_leaves_all_negzero<true>(q, 1u << (kk - 3u), t, zm) : wave_leaves_all_negzero<false>(q, 1u << (kk - 3u), t, zm));
                    goff += 1u << (kk - 3u);
                } else {
                    for (uint32_t l = 0; l < (1u << kk); ++l) {
                        const float2 pr = vparams[(size_t)goff * 8u + l];   // wave-uniform address
                        const float lf = fast ? bank_leaf<true, true>(t, pr.x, pr.y) : bank_leaf<false, true>(t, pr.x, pr.y);
                        ok = ok && __float_as_uint(lf) == 0x80000000u;
                    }
                    goff += 1u;
                }
            }
            if ((zm >> lane) & 1ull) orow[bank_out_index(a, ti)] = ok ? -0.0f : 0.0f;
            continue;
        }
        while (zm) {
            const uint32_t l = (uint32_t)__builtin_ctzll(zm);
            zm &= zm - 1;
            const uint64_t tz_i = (uint64_t)tile * 64u + l;
            const float tz = bank_time(a, tz_i);
            bool ok = true;
            uint32_t pair0 = 0;
            for (uint32_t i = 0; i < ni && ok; ++i) {
                const uint32_t kk = a.groups[i0 + i] & 15u, sz = 1u << kk;
                for (uint32_t q = lane; q < sz && ok; q += 64u) {
                    float2 p = vparams[pair0 + q];
                    ok = __float_as_uint(bank_leaf<false, true>(tz, p.x, p.y)) == 0x80000000u;
                }
                ok = __all(ok);
                pair0 += sz < 8u ? 8u : sz;
            }
            if (lane == 0) orow[bank_out_index(a, tz_i)] = ok ? -0.0f : 0.0f;
        }
    }
}

hipError_t launch_gbank(const BankArgs &a, hipStream_t s) {
    if (!a.groups || !a.group_off) return hipErrorInvalidValue;
    const uint64_t tiles = (a.n_times + 63) / 64;
    if (a.voices_per_wave) {   // many small voices: whole voices per wave
        if (a.voices_per_wave > 64) return hipErrorInvalidValue;
        const uint64_t nb = tiles * (((uint64_t)a.n_voices + 4ull * a.voices_per_wave - 1) / (4ull * a.voices_per_wave));
        if (nb == 0) return hipSuccess;
        if (nb > 0x7FFFFFFFull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(gbank_multi_kernel, dim3((uint32_t)nb), dim3(256), 0, s, a, (uint32_t)tiles, (uint32_t)nb);
        return hipGetLastError();
    }
    const uint64_t nblocks64 = tiles * a.n_voices;   // one workgroup (4 waves) per (voice, tile)
    if (nblocks64 == 0) return hipSuccess;
    if (nblocks64 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gbank_kernel, dim3((uint32_t)nblocks64), dim3(256), 0, s, a, (uint32_t)tiles, (uint32_t)nblocks64);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Staged evaluator: one thread per (program, frame).  Temporaries live in LDS as [register][thread] columns
// (conflict-free, no barriers: a thread only touches its own column).  Ring reads are the materialised
// form of the reference's "re-evaluate the source at t - d" (reference.rs:213-215): the ring holds exactly the
// values that re-evaluation would produce, because it was filled by the same graph from the same input history.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float stage_input(const StageArgs &a, uint32_t slot, uint64_t t) {
    if (slot >= a.n_inputs) return 0.0f;
    DevInput s = a.n_inputs <= STAGE_INLINE_INPUTS ? a.inline_inputs[slot] : a.inputs[slot];
    if (t < s.base || t >= s.len) return 0.0f;
    return s.data[t - s.base];
}

__device__ __forceinline__ float stage_load(const StageArgs &a, const StageInstr &in, uint64_t t) {
    switch (in.op) {
    case S_CONST: return __uint_as_float(in.imm);
    case S_INPUT: return stage_input(a, in.imm, t);
    case S_READ: return t >= in.d_lo ? a.rings[(size_t)in.buf * (a.ring_mask + 1) + ((t - in.d_lo) & a.ring_mask)] : 0.0f;
    case S_READ_INPUT: return t >= in.d_lo ? stage_input(a, in.imm, t - in.d_lo) : 0.0f;
    default: return t >= in.d_lo ? __uint_as_float(in.imm) : 0.0f;   // S_STEP
    }
}

__global__ void __launch_bounds__(256) stage_kernel(StageArgs a) {
    __shared__ float tmp[STAGE_REGS][256];
    // (kernels.hpp STAGE_CARRY: what this thread stored one iteration ago; dynamic LDS, only launches of feedback plans ask for it:
    //  the interpreter's 48 KB of registers already allow only three workgroups per CU)
    extern __shared__ float carry_mem[];
    auto carry = [&](uint32_t par, uint32_t slot) -> float & { return carry_mem[((size_t)par * STAGE_CARRY + slot) * 256u + threadIdx.x]; };
    const uint64_t wi0 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    // one frame per thread, or (stride != 0) the frames wi0, wi0 + stride, ... of the window in order: the planner's
    // fused_stride divides every delay with which this launch reads a ring it also writes, so a thread reads only what it
    // stored itself earlier in this loop, or an earlier launch did
    const uint64_t span = a.stride ? a.stride : a.w_len;
    if (wi0 >= span) return;
    const StageProg pg = a.progs[blockIdx.y];
    const uint32_t tid = threadIdx.x;
    const StageInstr *gins = a.instrs + pg.first_instr;
    auto fetch = [&](uint32_t i) -> StageInstr { return gins[i]; };
    uint32_t par = 0;
    for (uint64_t wi = wi0; wi < a.w_len; wi += span, par ^= 1u) {
    const uint64_t t = a.w0 + wi;
    const bool carried = wi != wi0 && a.use_carry != 0u;   // (the first iteration reads what an earlier launch stored)
    auto load = [&](const StageInstr &in) -> float {
        if (in.op == S_READ && in.imm != 0u && in.imm <= STAGE_CARRY && carried) return carry(par ^ 1u, in.imm - 1u);
        return stage_load(a, in, t);
    };
    // 1. the program's loads (ring reads at t - d, inputs, constants), all in flight together
    {
        float ld[STAGE_MAX_HOISTED];
#pragma unroll
        for (uint32_t i = 0; i < STAGE_MAX_HOISTED; ++i)
            if (i < pg.n_loads) ld[i] = load(fetch(i));
#pragma unroll
        for (uint32_t i = 0; i < STAGE_MAX_HOISTED; ++i)
            if (i < pg.n_loads) tmp[fetch(i).dst][tid] = ld[i];
    }
    // 2. everything else in program order.  The arithmetic is STAGE_ARITH_CASES; stage_sweep_kernel below repeats the rest of this
    //    step: this loop's time follows the compiler's output closely, see DESIGN 4.7 and profiles/stage_step.txt before sharing more
    for (uint32_t i = pg.n_loads; i < pg.n_instr; ++i) {
        const StageInstr in = fetch(i);
        float v;
        switch (in.op) {
        STAGE_ARITH_CASES(v, tmp[in.a][tid], tmp[in.b][tid], a.sparkle != 0u)
        case S_STORE:
            a.rings[(size_t)in.buf * (a.ring_mask + 1) + (t & a.ring_mask)] = tmp[in.a][tid];
            if (in.imm != 0u && in.imm <= STAGE_CARRY && a.use_carry) carry(par, in.imm - 1u) = tmp[in.a][tid];
            continue;
        case S_READ_DYN: case S_READ_INPUT_DYN: case S_STEP_DYN: {   // Delay by a signal amount (reference.rs:200-215)
            uint64_t fr;
            v = 0.0f;
            if (delay_frames(tmp[in.a][tid], fr, a.sparkle != 0u) && t >= fr) {
                if (in.op == S_READ_DYN) v = a.rings[(size_t)in.buf * (a.ring_mask + 1) + ((t - fr) & a.ring_mask)];
                else if (in.op == S_READ_INPUT_DYN) v = stage_input(a, in.imm, t - fr);
                else v = __uint_as_float(in.imm);
            }
            break;
        }
        default: v = load(in); break;   // a load that was not hoisted (register budget)
        }
        tmp[in.dst][tid] = v;
    }
    const float r = tmp[pg.result_reg][tid];
    if (pg.dst_ring != 0xFFFFFFFFu) a.rings[(size_t)pg.dst_ring * (a.ring_mask + 1) + (t & a.ring_mask)] = r;
    if (pg.out_row >= 0 && t >= a.idx) a.out[(size_t)pg.out_row * a.n_times + (t - a.idx)] = r;
    if (a.stride && !a.carry_only) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this stride's ring stores are in memory before the next one reads them
    }
}

// Loop tiles (kernels.hpp StageArgs::tile, callplan.hpp loop_tile): the strided launch of a feedback plan whose stride is at most
// 64 frames, ONE wave per program, the window rendered in tiles of a.tile frames (a multiple of the stride, so lane r < stride
// owns residue r in every tile).  stage_kernel keeps global memory inside its serial loop -- every operand a load from one
// active lane, every ring and row store a dword of its own, the range tests and ring addresses in 64-bit arithmetic per frame --
// and leaves the lanes >= stride idle.  Here a tile goes through three phases:
//   1. all 64 lanes, lane = frame: the loads that depend on the frame alone (S_INPUT, S_READ_INPUT, S_READ of a ring the
//      program does not store: imm == 0), range test applied, coalesced, into ldt[load slot][frame];
//   2. lanes < stride: the residue's frames in order, operands from ldt, own rings from the carry, everything stage_kernel
//      stores to a ring or a row into stt[store slot][frame] -- no global memory access but the instruction fetch;
//   3. all 64 lanes: stt to the rings and the output row, coalesced, under stage_kernel's conditions.
// Load slots number the frame-only loads in program order, store slots the S_STOREs in program order, then dst_ring, then
// out_row (tile_is_load; the walk of phase 2 counts as the set-up walk does, and clamps the slot: the rule admits programs of
// at most STAGE_TILE_LOADS loads and STAGE_TILE_STORES stores, the kernel stays in bounds without it).  No lane returns before
// the last barrier; every loop is bounded by w_len.
__device__ __forceinline__ bool tile_is_load(const StageInstr &in) {
    return in.op == S_INPUT || in.op == S_READ_INPUT || (in.op == S_READ && in.imm == 0u);
}

__global__ void __launch_bounds__(64) stage_tile_kernel(StageArgs a) {
    __shared__ float tmp[STAGE_REGS][64];
    __shared__ float ldt[STAGE_TILE_LOADS][STAGE_TILE_FRAMES];
    __shared__ float stt[STAGE_TILE_STORES][STAGE_TILE_FRAMES];
    __shared__ float cyt[2][STAGE_CARRY][64];
    __shared__ uint32_t ld_at[STAGE_TILE_LOADS];    // load slot -> instruction
    __shared__ uint32_t st_ring[STAGE_TILE_STORES]; // store slot -> ring
    const uint32_t lane = threadIdx.x;
    const StageProg pg = a.progs[blockIdx.y];
    const StageInstr *gins = a.instrs + pg.first_instr;
    const uint32_t stride = (uint32_t)a.stride, tile = a.tile;
    const size_t ring_cap = (size_t)a.ring_mask + 1;
    // set-up: the slot tables (every lane counts -- the counts are uniform --, lane 0 writes), and the carry's first values: what
    // an earlier launch left in the rings `stride` frames before the lane's first frame, or +0
    uint32_t n_ld = 0, n_st = 0;
    for (uint32_t i = 0; i < pg.n_instr; ++i) {
        const StageInstr in = gins[i];
        if (tile_is_load(in)) {
            if (lane == 0 && n_ld < STAGE_TILE_LOADS) ld_at[n_ld] = i;
            ++n_ld;
        } else if (in.op == S_STORE) {
            if (lane == 0 && n_st < STAGE_TILE_STORES) st_ring[n_st] = in.buf;
            ++n_st;
        } else if (in.op == S_READ && in.imm <= STAGE_CARRY && lane < stride && lane < a.w_len) {
            cyt[1][in.imm - 1u][lane] = stage_load(a, in, a.w0 + lane);
        }
    }
    if (pg.dst_ring != 0xFFFFFFFFu) {
        if (lane == 0 && n_st < STAGE_TILE_STORES) st_ring[n_st] = pg.dst_ring;
        ++n_st;
    }
    n_ld = n_ld < STAGE_TILE_LOADS ? n_ld : STAGE_TILE_LOADS;
    n_st = n_st < STAGE_TILE_STORES ? n_st : STAGE_TILE_STORES;                 // ring stores; the row's slot follows them
    const uint32_t row_slot = n_st < STAGE_TILE_STORES ? n_st : STAGE_TILE_STORES - 1u;
    __syncthreads();
    uint32_t par = 0;
    for (uint64_t base = 0; base < a.w_len; base += tile) {
        const uint32_t n = (uint32_t)(a.w_len - base < tile ? a.w_len - base : tile);   // frames of this tile
        // 1. the tile's frame-only loads, a frame's in flight together
        for (uint32_t f = lane; f < n; f += 64u) {
            const uint64_t t = a.w0 + base + f;
            float ld[STAGE_TILE_LOADS];
#pragma unroll
            for (uint32_t k = 0; k < STAGE_TILE_LOADS; ++k)
                if (k < n_ld) ld[k] = stage_load(a, gins[ld_at[k]], t);
#pragma unroll
            for (uint32_t k = 0; k < STAGE_TILE_LOADS; ++k)
                if (k < n_ld) ldt[k][f] = ld[k];
        }
        __syncthreads();
        // 2. the loops, a lane per residue
        if (lane < stride) {
            for (uint32_t f = lane; f < n; f += stride, par ^= 1u) {
                uint32_t k = 0, s = 0;
                for (uint32_t i = 0; i < pg.n_instr; ++i) {
                    const StageInstr in = gins[i];
                    float v;
                    switch (in.op) {
                    case S_CONST: v = __uint_as_float(in.imm); break;
                    case S_INPUT: case S_READ_INPUT: v = ldt[k++ & (STAGE_TILE_LOADS - 1u)][f]; break;
                    case S_READ:
                        if (in.imm == 0u) v = ldt[k++ & (STAGE_TILE_LOADS - 1u)][f];
                        else v = cyt[par ^ 1u][(in.imm - 1u) & (STAGE_CARRY - 1u)][lane];
                        break;
                    case S_STEP: v = a.w0 + base + f >= in.d_lo ? __uint_as_float(in.imm) : 0.0f; break;
                    STAGE_ARITH_CASES(v, tmp[in.a][lane], tmp[in.b][lane], a.sparkle != 0u)
                    case S_STORE:
                        stt[s < STAGE_TILE_STORES ? s : STAGE_TILE_STORES - 1u][f] = tmp[in.a][lane];
                        ++s;
                        if (in.imm != 0u && in.imm <= STAGE_CARRY) cyt[par][in.imm - 1u][lane] = tmp[in.a][lane];
                        continue;
                    default: v = 0.0f; break;   // (a Delay of a signal amount: the rule tiles no such program)
                    }
                    tmp[in.dst][lane] = v;
                }
                const float r = tmp[pg.result_reg][lane];
                if (pg.dst_ring != 0xFFFFFFFFu) stt[n_st - 1u][f] = r;
                if (pg.out_row >= 0) stt[row_slot][f] = r;
            }
        }
        __syncthreads();   // (also: phase 2 has read ldt before the next tile's phase 1 overwrites it)
        // 3. the tile's stores
        for (uint32_t f = lane; f < n; f += 64u) {
            const uint64_t t = a.w0 + base + f;
#pragma unroll
            for (uint32_t k = 0; k < STAGE_TILE_STORES; ++k)
                if (k < n_st) a.rings[(size_t)st_ring[k] * ring_cap + (t & a.ring_mask)] = stt[k][f];
            if (pg.out_row >= 0 && t >= a.idx) a.out[(size_t)pg.out_row * a.n_times + (t - a.idx)] = stt[row_slot][f];
        }
        // (phase 3 reads stt, the next tile's phase 2 writes it: the barrier after its phase 1 stands between them)
    }
}

hipError_t launch_stage(const StageArgs &a, hipStream_t s) {
    if (a.n_progs == 0 || a.w_len == 0) return hipSuccess;
    if (a.n_progs > 65535u) return hipErrorInvalidValue;
    if (a.tile) {
        if (a.stride == 0 || a.stride > 64 || a.tile > STAGE_TILE_FRAMES || a.tile % a.stride != 0) return hipErrorInvalidValue;
        hipLaunchKernelGGL(stage_tile_kernel, dim3(1, a.n_progs), dim3(64), 0, s, a);
        return hipGetLastError();
    }
    uint64_t bx = ((a.stride ? std::min(a.stride, a.w_len) : a.w_len) + 255) / 256;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const size_t carry_bytes = a.use_carry ? (size_t)2 * STAGE_CARRY * 256 * sizeof(float) : 0;
    hipLaunchKernelGGL(stage_kernel, dim3((uint32_t)bx, a.n_progs), dim3(256), carry_bytes, s, a);
    return hipGetLastError();
}

// Sweeps (kernels.hpp launch_stage_sweep, callplan.hpp loop_sweep): a feedback plan whose loops delay by a signal amount has no
// stride that binds a thread to its own stores, but a proven bound: every read of a ring the program stores reaches at least
// a.sweep frames back.  ONE workgroup per program walks the window a.sweep frames at a time, thread = frame of the sweep, each
// thread the whole program for its frame exactly as stage_kernel runs it (stage_load, delay_frames, STAGE_ARITH_CASES, the
// S_*_DYN case, the same stores under the same conditions).  Between two sweeps every thread waits for its own stores
// (s_waitcnt vmcnt(0): on gfx950 stores count there) and the workgroup passes a barrier: the waves of a workgroup share their
// CU's vector cache, which writes through, so a plain load after the barrier sees a plain store from before it.  Every thread
// reaches every barrier -- the loop's bounds are uniform, threads beyond the sweep's frames only skip the work --, every loop
// is bounded by w_len, nothing polls.  A workgroup of one wave (sweep <= 64) pays the wait alone: its barrier has nobody to wait for.
__global__ void __launch_bounds__(256) stage_sweep_kernel(StageArgs a) {
    __shared__ float tmp[STAGE_REGS][256];
    const StageProg pg = a.progs[blockIdx.y];
    const uint32_t tid = threadIdx.x;
    const StageInstr *gins = a.instrs + pg.first_instr;
    const size_t ring_cap = (size_t)a.ring_mask + 1;
    const uint32_t sweep = a.sweep;
    for (uint64_t base = 0; base < a.w_len; base += sweep) {
        const uint64_t left = a.w_len - base;
        if (tid < sweep && tid < left) {
            const uint64_t t = a.w0 + base + tid;
            {   // 1. the program's hoisted loads, in flight together
                float ld[STAGE_MAX_HOISTED];
#pragma unroll
                for (uint32_t i = 0; i < STAGE_MAX_HOISTED; ++i)
                    if (i < pg.n_loads) ld[i] = stage_load(a, gins[i], t);
#pragma unroll
                for (uint32_t i = 0; i < STAGE_MAX_HOISTED; ++i)
                    if (i < pg.n_loads) tmp[gins[i].dst][tid] = ld[i];
            }
            // 2. everything else in program order
            for (uint32_t i = pg.n_loads; i < pg.n_instr; ++i) {
                const StageInstr in = gins[i];
                float v;
                switch (in.op) {
                STAGE_ARITH_CASES(v, tmp[in.a][tid], tmp[in.b][tid], a.sparkle != 0u)
                case S_STORE: a.rings[(size_t)in.buf * ring_cap + (t & a.ring_mask)] = tmp[in.a][tid]; continue;
                case S_READ_DYN: case S_READ_INPUT_DYN: case S_STEP_DYN: {   // Delay by a signal amount (reference.rs:200-215)
                    uint64_t fr;
                    v = 0.0f;
                    if (delay_frames(tmp[in.a][tid], fr, a.sparkle != 0u) && t >= fr) {
                        if (in.op == S_READ_DYN) v = a.rings[(size_t)in.buf * ring_cap + ((t - fr) & a.ring_mask)];
                        else if (in.op == S_READ_INPUT_DYN) v = stage_input(a, in.imm, t - fr);
                        else v = __uint_as_float(in.imm);
                    }
                    break;
                }
                default: v = stage_load(a, in, t); break;   // a load that was not hoisted (register budget)
                }
                tmp[in.dst][tid] = v;
            }
            const float r = tmp[pg.result_reg][tid];
            if (pg.dst_ring != 0xFFFFFFFFu) a.rings[(size_t)pg.dst_ring * ring_cap + (t & a.ring_mask)] = r;
            if (pg.out_row >= 0 && t >= a.idx) a.out[(size_t)pg.out_row * a.n_times + (t - a.idx)] = r;
        }
        // the sweep's ring stores are in memory before any thread of the workgroup starts the next sweep
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

hipError_t launch_stage_sweep(const StageArgs &a, hipStream_t s) {
    if (a.n_progs == 0 || a.w_len == 0) return hipSuccess;
    if (a.n_progs > 65535u || a.sweep == 0 || a.sweep > STAGE_SWEEP_MAX || a.stride != 0 || a.tile != 0 || a.use_carry != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stage_sweep_kernel, dim3(1, a.n_progs), dim3(64u * ((a.sweep + 63u) / 64u)), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// The sixteen resident kernels (kernels.hpp StreamKernel; the pieces and the protocol: above, "Block streaming"): ONE body,
// stream_resident_body, instantiated by the kernel's form (kernels.hpp StreamForm).  The body is the protocol's skeleton -- when
// `alive` is published, the block loop and its stop test, which wave counts a voice in, when LDS may be reused -- and every
// kernel is the one before it and one thing more:
//
//   kernel                       adds                                                              LDS bytes
//   bank_stream_kernel           banks alone: one-row doorbell, the finished voice to its host row     4 112
//   bank_stream_prog_kernel      the voices' programs (StreamProgArgs), `head`; registers in LDS      16 400
//   bank_stream_bus_kernel       the bus segment in the block's last arriver                          16 400
//   bank_stream_in_kernel        a doorbell of n_rows rows, S_INPUT by row                            16 400
//   bank_stream_banks_kernel     a workgroup finds its bank in the bank table                         16 400
//   bank_stream_loops_kernel     loop programs in three phases (stream_run_loop_program)              36 880
//   bank_stream_general_kernel   schedule banks (stream_render_schedule)                              45 072
//   bank_stream_dyn_kernel       Delays by a signal amount (stream_prog_dyn)                          45 072
//   bank_stream_hist_kernel      delayed reads of input rows: the rows' history (StreamHistArgs)      45 072
//   bank_stream_store_kernel     the streamed rows appended to the input store (StreamStoreArgs)      45 072
//
// and, beside the cascade, the form without a voice (kernels.hpp bank_stream_fx_kernel): the hist form's programs, doorbell and
// history with no bank, no render and no hand-over -- a workgroup is ONE wave that runs a segment of programs  32 776
// (bank_stream_store_fx_kernel: the same, and the streamed rows appended to the input store                 32 776)
// and the four sweep forms (kernels.hpp bank_stream_sweep_kernel): the hist, fx, store and store_fx forms whose loop programs walk
// the block in sweeps and know the Delays by a signal amount (stream_run_loop_program<true>); LDS as the form underneath.
// And the two leaf forms (kernels.hpp bank_stream_leaf_kernel): the hist and the store form whose leaf banks -- compiled voices --
// are rendered by the leaf interpreter (stream_render_leaves); LDS: the form's 45 072 + 32 768 of registers + 2 048 of rows = 79 888.
// And the two track forms (kernels.hpp bank_stream_track_kernel): the leaf forms whose leaves read track rows of the block's staged
// matrix, one partial ahead; LDS: the leaf form's 79 888 + 32 768 of parked rows = 112 656.
//
// The bus segment is progs[voice_first[n_voices] .. voice_first[n_voices + 1]) and may be empty.  Which kernel a plan launches
// is the host's rule (streamplan.hpp; fr_plan_json["stream"]["kernel"]).  The compiled kernels against their earlier,
// separately written text: profiles/stream_resident_body.txt.
// ---------------------------------------------------------------------------------------------------

// S_INPUT of the one-row kernels: the block's row, which the finishing wave holds as `t`.
struct StreamRowInput {
    static constexpr bool history = false;
    float t;
    __device__ __forceinline__ float operator()(uint32_t) const { return t; }
};
// S_INPUT of the control-row kernels.  imm is the streamed row (the host rewrote it); rows the launch does not stream hold +0.0.
// Row 0 is `t`; the others were republished before this workgroup saw the block's seq: a relaxed agent-scope load, in flight
// with the program's other leading loads.
struct StreamRowsInput {
    static constexpr bool history = false;
    const BankStreamInDev *dev;
    uint32_t lane;
    float t;
    __device__ __forceinline__ float operator()(uint32_t row) const {
        return row == 0u ? t : __hip_atomic_load(&dev->rows[row & (BANK_STREAM_ROWS - 1u)][lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// The hist form (kernels.hpp bank_stream_hist_kernel, where the argument for all of this stands).  The history of the streamed
// rows is hist[row][frame & hmask].  StreamHistoryStore is workgroup 0's side: wave 0 stores the live lanes of every row of the
// block at `head` right after it has republished them -- relaxed agent-scope VECTOR stores, acknowledged by the wait's one
// s_waitcnt vmcnt(0) together with the rows, so before n_times and seq.  StreamHistInput is the readers' side: S_INPUT as
// StreamRowsInput, `at` a row's sample of an absolute frame -- a relaxed agent-scope load (L2's copy, never a CU's L1: the
// storer is another CU), row and index masked.
struct StreamHistoryStore {
    float *hist;
    uint64_t hmask, head;
    uint32_t lane;
    __device__ __forceinline__ void operator()(uint32_t row, float v, uint32_t T) const {
        if (lane < T) __hip_atomic_store(hist + (size_t)row * (hmask + 1) + ((head + lane) & hmask), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
// The store forms (kernels.hpp bank_stream_store_kernel): the hist form's Keep, and the same lanes of the same words appended to
// the renderer's input store -- one more relaxed agent-scope VECTOR store per streamed row under the wait's one acknowledgement.
// `row` is a constant of the unrolled wait, so s.row[row] is a pair of registers; a slot without a buffer is a uniform skip.
struct StreamStoreKeep {
    StreamHistoryStore hist;
    StreamStoreArgs s;
    __device__ __forceinline__ void operator()(uint32_t row, float v, uint32_t T) const {
        hist(row, v, T);
        float *const data = s.row[row].data;
        if (data != nullptr && hist.lane < T) __hip_atomic_store(data + (hist.head + hist.lane - s.row[row].base), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct StreamHistInput {
    static constexpr bool history = true;
    StreamRowsInput rows;
    const float *hist;
    uint64_t hmask;
    __device__ __forceinline__ float operator()(uint32_t row) const { return rows(row); }
    __device__ __forceinline__ float at(uint32_t row, uint64_t frame) const {
        return __hip_atomic_load(hist + (size_t)(row & (BANK_STREAM_ROWS - 1u)) * (hmask + 1) + (frame & hmask), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// What the doorbell's form decides, by overload on its device block: workgroup 0's wait, the block's time row, S_INPUT.
template <class Keep>
__device__ __forceinline__ uint32_t stream_doorbell_wait(uint32_t, BankStreamCtl *ctl, BankStreamDev *dev, uint32_t lane, uint32_t seen, unsigned long long idle_ticks,
                                                         uint32_t &T, const Keep &) {
    return stream_row_wait(ctl, dev, lane, seen, idle_ticks, T);
}
template <class Keep>
__device__ __forceinline__ uint32_t stream_doorbell_wait(uint32_t n_rows, BankStreamInCtl *ctl, BankStreamInDev *dev, uint32_t lane, uint32_t seen,
                                                         unsigned long long idle_ticks, uint32_t &T, const Keep &keep) {
    return stream_rows_wait(n_rows, ctl, dev, lane, seen, idle_ticks, T, keep);
}
__device__ __forceinline__ const float *stream_time_row(const BankStreamDev *dev) { return dev->row; }
__device__ __forceinline__ const float *stream_time_row(const BankStreamInDev *dev) { return dev->rows[0]; }
__device__ __forceinline__ StreamRowInput stream_input(const BankStreamDev *, uint32_t, float t) { return {t}; }
__device__ __forceinline__ StreamRowsInput stream_input(const BankStreamInDev *dev, uint32_t lane, float t) { return {dev, lane, t}; }

// The resident kernel of form K.  The argument structs come BY VALUE (by reference the bank table goes to scratch); what a form
// does not have is passed empty and never read, and a __shared__ array it does not use takes no LDS.
//
// A workgroup's bank is the last one of the table whose first workgroup is not after it (the table is in ascending order; the
// grid is exactly the sum of the banks' workgroups), found once, uniformly, before the block loop; without a table it is the
// one bank of BankArgs.  Voices are numbered globally: chunk sums, tickets, voice_first and the voices_done count -- whichever
// bank the block's last arriver is of -- all go by that number.  A workgroup of a schedule bank renders the voice first_voice +
// (blockIdx.x - first_wg) whole: its chunk count is 1, so stream_hand_over returns at once.
static_assert(STREAM_STACK_DEPTH == GB_MAX_DEPTH, "a schedule voice's stack is the general voices'");
template <StreamKernel K, class Ctl, class Dev>
__device__ __forceinline__ void stream_resident_body(StreamBanksArgs t, StreamGeneralArgs g, StreamHistArgs h, StreamStoreArgs st, StreamLeafArgs lf, StreamTrackArgs tk, BankArgs a, StreamProgArgs p,
                                                     uint32_t n_rows, Ctl *ctl, Dev *dev, uint32_t idle_ms) {
    constexpr StreamForm F = stream_form(K);
    __shared__ float sm[F.schedule ? 2 : 1][STREAM_NW][64];  // the waves' sums: a chunk's in [0], a schedule's items alternate
    __shared__ float stack_mem[STREAM_STACK_DEPTH][64];      // a schedule voice's evaluation stack: [level][frame] of wave 0
    __shared__ float regs[STAGE_REGS][64];                   // the interpreter's registers: [register][frame] of wave 0
    __shared__ float ldt[BANK_STREAM_LOOP_LOADS][64];        // a loop program's loads, [load slot][frame]
    __shared__ float stt[BANK_STREAM_LOOP_STORES][64];       // ... and what it stores to its rings, [store slot][frame]
    __shared__ uint4 lins[BANK_STREAM_LOOP_INSTRS];          // ... and its (first) instructions
    __shared__ float lregs[STREAM_NW][BANK_STREAM_LEAF_REGS][64];   // the leaf interpreter's registers: [wave][register][frame] (leaf forms only)
    __shared__ float lin[BANK_STREAM_ROWS][64];              // ... and the block's streamed rows, [row][frame]
    __shared__ float ltrk[STREAM_NW][2][BANK_STREAM_LEAF_TRACKS][64];   // the parked track rows: [wave][partial & 1][track][frame] (track forms only)
    __shared__ unsigned long long zshared;
    __shared__ uint32_t s_seq, s_T;
    StreamBanksArgs::Bank bk = {a.params, a.rows, 0u, 0u, a.n_voices, a.log2_p, a.chunk_log2, a.fast_ok, p.bank_to_ring};
    const uint32_t *groups = nullptr, *group_off = nullptr;
    uint32_t bi = 0;
    if constexpr (F.table) {
        bk = t.bank[0];
        groups = g.bank[0].groups;
        group_off = g.bank[0].group_off;
        static_for<1, (int)BANK_STREAM_BANKS>([&](auto j) {
            if ((uint32_t)j < t.n_banks && blockIdx.x >= t.bank[j].first_wg) {
                bk = t.bank[j];
                groups = g.bank[j].groups;
                group_off = g.bank[j].group_off;
                bi = (uint32_t)j;
            }
        });
    }
    const bool schedule = F.schedule && ((g.mask >> bi) & 1u);   // uniform: the workgroup's bank is a schedule bank
    [[maybe_unused]] bool leaves = false;                        // uniform: ... or a leaf bank (the leaf forms only)
    [[maybe_unused]] StreamLeafArgs::Bank lb = {};
    if constexpr (F.leaf) {
        leaves = (lf.mask >> bi) & 1u;
        lb = lf.bank[0];
        static_for<1, (int)BANK_STREAM_BANKS>([&](auto j) {
            if (bi == (uint32_t)j) lb = lf.bank[j];
        });
    }
    [[maybe_unused]] StreamTrackWave tw = {};                    // ... and its leaf's track rows (the track forms only)
    if constexpr (F.tracks) {
        tw = {tk.staging, tk.first_slot, tk.rows, tk.bank[0], lb.k};
        static_for<1, (int)BANK_STREAM_BANKS>([&](auto j) {
            if (bi == (uint32_t)j) tw.tb = tk.bank[j];
        });
    }
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t local = blockIdx.x - bk.first_wg;
    // (a schedule bank: log2_p = chunk_log2 = 0 makes `local` the voice of the bank and its chunk count 1)
    // (the voiceless form has no bank: nothing to render, a workgroup's work is its segment of programs)
    const StreamWork w = F.voiceless ? StreamWork{}
                                     : stream_work(bk.params, bk.rows, schedule ? 0u : bk.log2_p, schedule ? 0u : bk.chunk_log2, bk.fast_ok, bk.to_ring, bk.first_voice, local, wave);
    const uint32_t *items = nullptr;
    const float *vparams = nullptr;
    uint32_t nitems = 0;
    if (schedule) {
        typedef uint32_t __attribute__((address_space(4))) const *const_u32_ptr;
        const_u32_ptr go = (const_u32_ptr)group_off;
        const uint32_t i0 = go[2u * local];
        nitems = go[2u * local + 2u] - i0;
        items = groups + i0;
        vparams = (const float *)(bk.params + (size_t)go[2u * local + 1u] * 8u);
    }
    const uint32_t n_voices = a.n_voices;                    // of all banks
    const unsigned long long idle_ticks = (unsigned long long)idle_ms * 100000ull;
    uint64_t head = p.head;                                  // the first frame of the block, the same in every workgroup
    uint32_t seen = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(&ctl->alive, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    for (;;) {
        uint32_t T;
        const uint32_t seq = stream_next_block(dev, wave, lane, seen, idle_ticks, s_seq, s_T, T, [&](uint32_t &T0) {
            // (the hist form: workgroup 0 keeps the block's rows, at the `head` every workgroup of a progs form carries)
            // (the store forms: and appends them to the input store, under the same acknowledgement)
            if constexpr (F.store) return stream_doorbell_wait(n_rows, ctl, dev, lane, seen, idle_ticks, T0, StreamStoreKeep{{h.hist, h.mask, head, lane}, st});
            else if constexpr (F.hist) return stream_doorbell_wait(n_rows, ctl, dev, lane, seen, idle_ticks, T0, StreamHistoryStore{h.hist, h.mask, head, lane});
            else return stream_doorbell_wait(n_rows, ctl, dev, lane, seen, idle_ticks, T0, StreamNoHistory{});
        });
        if (seq == BANK_STREAM_STOP) break;
        seen = seq;
        const bool live = lane < T;
        if constexpr (F.voiceless) {
            // no voice: the workgroup is one wave, its segment's programs are the block's work (kernels.hpp bank_stream_fx_kernel).
            // S_INPUT(0) is the lane's word of the republished time row, as the rendering waves of the other forms load it.
            const float t_row = live ? __hip_atomic_load(&stream_time_row(dev)[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
            const StreamHistInput input{stream_input(dev, lane, t_row), h.hist, h.mask};
            auto run = [&](uint32_t p_first, uint32_t p_end) {
                if constexpr (F.sweep) stream_run_programs_loops<true, true>(a.out, p, regs, ldt, stt, lins, p_first, p_end, head, T, lane, live, input);
                else stream_run_programs_loops<true>(a.out, p, regs, ldt, stt, lins, p_first, p_end, head, T, lane, live, input);
            };
            run(p.voice_first[blockIdx.x], p.voice_first[blockIdx.x + 1u]);
            stream_finish_bus(ctl, dev, n_voices, lane, seq, [&] { run(p.voice_first[n_voices], p.voice_first[n_voices + 1u]); });
        } else {
            float t_in, result, r;
            // (the conditional expression the general kernel has always had: as an if / else its compiled loop comes out another)
            if constexpr (F.tracks)
                r = leaves     ? stream_render_leaves<true>(w, bk, lb, dev, n_rows, p.sparkle != 0u, live, wave, lane, sm[0], lregs, lin, t_in, tw, &ctl->tracks, ltrk)
                    : schedule ? stream_render_schedule(vparams, items, nitems, bk.fast_ok, stream_time_row(dev), live, wave, lane, sm, stack_mem, zshared, t_in)
                               : stream_render_chunk(w, stream_time_row(dev), live, wave, lane, sm[0], zshared, t_in);
            else if constexpr (F.leaf)
                r = leaves     ? stream_render_leaves(w, bk, lb, dev, n_rows, p.sparkle != 0u, live, wave, lane, sm[0], lregs, lin, t_in)
                    : schedule ? stream_render_schedule(vparams, items, nitems, bk.fast_ok, stream_time_row(dev), live, wave, lane, sm, stack_mem, zshared, t_in)
                               : stream_render_chunk(w, stream_time_row(dev), live, wave, lane, sm[0], zshared, t_in);
            else if constexpr (F.schedule)
                r = schedule ? stream_render_schedule(vparams, items, nitems, bk.fast_ok, stream_time_row(dev), live, wave, lane, sm, stack_mem, zshared, t_in)
                             : stream_render_chunk(w, stream_time_row(dev), live, wave, lane, sm[0], zshared, t_in);
            else r = stream_render_chunk(w, stream_time_row(dev), live, wave, lane, sm[0], zshared, t_in);
            if (wave == 0u && stream_hand_over(w, a.ws, a.tickets, n_voices, lane, r, result)) {
                // the finishing wave: the voice's frames head + lane to its ring or row, then its programs, then it counts the voice in
                const auto input = [&] {
                    if constexpr (F.hist) return StreamHistInput{stream_input(dev, lane, t_in), h.hist, h.mask};
                    else return stream_input(dev, lane, t_in);
                }();
                auto run = [&](uint32_t p_first, uint32_t p_end) {
                    if constexpr (F.sweep) stream_run_programs_loops<true, true>(a.out, p, regs, ldt, stt, lins, p_first, p_end, head, T, lane, live, input);
                    else if constexpr (F.loops) stream_run_programs_loops<F.dyn>(a.out, p, regs, ldt, stt, lins, p_first, p_end, head, T, lane, live, input);
                    else if constexpr (F.progs) stream_run_programs(a.out, p, regs, p_first, p_end, head + lane, lane, live, input);
                };
                stream_store_voice(w, a.out, p, head + lane, lane, live, result);
                if constexpr (F.progs) run(p.voice_first[w.voice], p.voice_first[w.voice + 1]);
                if constexpr (F.bus) stream_finish_bus(ctl, dev, n_voices, lane, seq, [&] { run(p.voice_first[n_voices], p.voice_first[n_voices + 1]); });
                else stream_finish(ctl, dev, n_voices, lane, seq);
            }
        }
        head += T;
        __syncthreads();   // LDS is reused by the next block
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(&ctl->alive, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void __launch_bounds__(1024) bank_stream_kernel(BankArgs a, BankStreamCtl *ctl, BankStreamDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::plain>({}, {}, {}, {}, {}, {}, a, {}, 1u, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_prog_kernel(BankArgs a, StreamProgArgs p, BankStreamCtl *ctl, BankStreamDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::prog>({}, {}, {}, {}, {}, {}, a, p, 1u, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_bus_kernel(BankArgs a, StreamProgArgs p, BankStreamCtl *ctl, BankStreamDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::bus>({}, {}, {}, {}, {}, {}, a, p, 1u, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_in_kernel(BankArgs a, StreamProgArgs p, uint32_t n_rows, BankStreamInCtl *ctl, BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::in>({}, {}, {}, {}, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_banks_kernel(StreamBanksArgs t, BankArgs a, StreamProgArgs p, uint32_t n_rows, BankStreamInCtl *ctl,
                                                                 BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::banks>(t, {}, {}, {}, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_loops_kernel(StreamBanksArgs t, BankArgs a, StreamProgArgs p, uint32_t n_rows, BankStreamInCtl *ctl,
                                                                 BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::loops>(t, {}, {}, {}, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_general_kernel(StreamBanksArgs t, StreamGeneralArgs g, BankArgs a, StreamProgArgs p, uint32_t n_rows, BankStreamInCtl *ctl,
                                                                   BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::general>(t, g, {}, {}, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_dyn_kernel(StreamBanksArgs t, StreamGeneralArgs g, BankArgs a, StreamProgArgs p, uint32_t n_rows, BankStreamInCtl *ctl,
                                                               BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::dyn>(t, g, {}, {}, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_hist_kernel(StreamBanksArgs t, StreamGeneralArgs g, StreamHistArgs h, BankArgs a, StreamProgArgs p, uint32_t n_rows,
                                                                BankStreamInCtl *ctl, BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::hist>(t, g, h, {}, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}
// (LAUNCHED with one wave per workgroup: a segment of programs needs no more, and nothing is rendered.  The bound stays the other
// forms': under __launch_bounds__(64) the compiler sees that 32 KiB of LDS leave room for one wave per SIMD and pads the wave's
// register allocation to 257 VGPRs to say so; with this bound it records the 48 the code uses)
__global__ void __launch_bounds__(1024) bank_stream_fx_kernel(StreamHistArgs h, BankArgs a, StreamProgArgs p, uint32_t n_rows, BankStreamInCtl *ctl, BankStreamInDev *dev,
                                                            uint32_t idle_ms) {
    stream_resident_body<StreamKernel::fx>({}, {}, h, {}, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}

// The store forms (kernels.hpp StreamStoreArgs): the hist form and the fx form, whose workgroup 0 also appends the streamed rows to
// the input store.
__global__ void __launch_bounds__(1024) bank_stream_store_kernel(StreamBanksArgs t, StreamGeneralArgs g, StreamHistArgs h, StreamStoreArgs st, BankArgs a, StreamProgArgs p,
                                                                 uint32_t n_rows, BankStreamInCtl *ctl, BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::store>(t, g, h, st, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_store_fx_kernel(StreamHistArgs h, StreamStoreArgs st, BankArgs a, StreamProgArgs p, uint32_t n_rows, BankStreamInCtl *ctl,
                                                                    BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::store_fx>({}, {}, h, st, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}

// The leaf forms (kernels.hpp bank_stream_leaf_kernel): the hist form and the store form whose leaf banks -- compiled voices -- are
// rendered by the leaf interpreter (stream_render_leaves).
__global__ void __launch_bounds__(1024) bank_stream_leaf_kernel(StreamBanksArgs t, StreamGeneralArgs g, StreamHistArgs h, StreamLeafArgs lf, BankArgs a, StreamProgArgs p,
                                                                uint32_t n_rows, BankStreamInCtl *ctl, BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::leaf>(t, g, h, {}, lf, {}, a, p, n_rows, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_leaf_store_kernel(StreamBanksArgs t, StreamGeneralArgs g, StreamHistArgs h, StreamStoreArgs st, StreamLeafArgs lf, BankArgs a,
                                                                      StreamProgArgs p, uint32_t n_rows, BankStreamInCtl *ctl, BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::leaf_store>(t, g, h, st, lf, {}, a, p, n_rows, ctl, dev, idle_ms);
}

// The track forms (kernels.hpp bank_stream_track_kernel): the leaf forms whose leaves read track rows of the block's staged matrix.
__global__ void __launch_bounds__(1024) bank_stream_track_kernel(StreamBanksArgs t, StreamGeneralArgs g, StreamHistArgs h, StreamLeafArgs lf, StreamTrackArgs tk, BankArgs a,
                                                                 StreamProgArgs p, uint32_t n_rows, BankStreamInCtl *ctl, BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::track>(t, g, h, {}, lf, tk, a, p, n_rows, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_track_store_kernel(StreamBanksArgs t, StreamGeneralArgs g, StreamHistArgs h, StreamStoreArgs st, StreamLeafArgs lf,
                                                                       StreamTrackArgs tk, BankArgs a, StreamProgArgs p, uint32_t n_rows, BankStreamInCtl *ctl,
                                                                       BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::track_store>(t, g, h, st, lf, tk, a, p, n_rows, ctl, dev, idle_ms);
}

// The sweep forms (kernels.hpp bank_stream_sweep_kernel): the hist, fx, store and store_fx forms whose loop programs walk sweeps.
__global__ void __launch_bounds__(1024) bank_stream_sweep_kernel(StreamBanksArgs t, StreamGeneralArgs g, StreamHistArgs h, BankArgs a, StreamProgArgs p, uint32_t n_rows,
                                                                 BankStreamInCtl *ctl, BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::sweep>(t, g, h, {}, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_sweep_fx_kernel(StreamHistArgs h, BankArgs a, StreamProgArgs p, uint32_t n_rows, BankStreamInCtl *ctl, BankStreamInDev *dev,
                                                                    uint32_t idle_ms) {
    stream_resident_body<StreamKernel::sweep_fx>({}, {}, h, {}, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_sweep_store_kernel(StreamBanksArgs t, StreamGeneralArgs g, StreamHistArgs h, StreamStoreArgs st, BankArgs a,
                                                                       StreamProgArgs p, uint32_t n_rows, BankStreamInCtl *ctl, BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::sweep_store>(t, g, h, st, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}
__global__ void __launch_bounds__(1024) bank_stream_sweep_store_fx_kernel(StreamHistArgs h, StreamStoreArgs st, BankArgs a, StreamProgArgs p, uint32_t n_rows,
                                                                          BankStreamInCtl *ctl, BankStreamInDev *dev, uint32_t idle_ms) {
    stream_resident_body<StreamKernel::sweep_store_fx>({}, {}, h, st, {}, {}, a, p, n_rows, ctl, dev, idle_ms);
}

// The one entry of the resident launches (kernels.hpp StreamLaunchArgs): the check, then the kernel with what it takes.
hipError_t launch_bank_stream(StreamKernel k, const StreamLaunchArgs &x, hipStream_t s) {
    const uint32_t wgs = stream_launch_check(k, x);
    if (!wgs) return hipErrorInvalidValue;
    BankStreamCtl *const ctl = static_cast<BankStreamCtl *>(x.ctl_dev);          // (the doorbell's form is the kernel's: StreamForm::rows)
    BankStreamDev *const dev = static_cast<BankStreamDev *>(x.dev);
    BankStreamInCtl *const ctl_in = static_cast<BankStreamInCtl *>(x.ctl_dev);
    BankStreamInDev *const dev_in = static_cast<BankStreamInDev *>(x.dev);
    const dim3 grid(wgs), block(1024), wave(64);   // (the voiceless form: a workgroup is one wave)
    const uint32_t idle_ms = x.idle_ms ? x.idle_ms : BANK_STREAM_IDLE_MS;
    switch (k) {
    case StreamKernel::plain: hipLaunchKernelGGL(bank_stream_kernel, grid, block, 0, s, x.a, ctl, dev, idle_ms); break;
    case StreamKernel::prog: hipLaunchKernelGGL(bank_stream_prog_kernel, grid, block, 0, s, x.a, x.p, ctl, dev, idle_ms); break;
    case StreamKernel::bus: hipLaunchKernelGGL(bank_stream_bus_kernel, grid, block, 0, s, x.a, x.p, ctl, dev, idle_ms); break;
    case StreamKernel::in: hipLaunchKernelGGL(bank_stream_in_kernel, grid, block, 0, s, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::banks: hipLaunchKernelGGL(bank_stream_banks_kernel, grid, block, 0, s, x.t, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::loops: hipLaunchKernelGGL(bank_stream_loops_kernel, grid, block, 0, s, x.t, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::general: hipLaunchKernelGGL(bank_stream_general_kernel, grid, block, 0, s, x.t, x.g, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::dyn: hipLaunchKernelGGL(bank_stream_dyn_kernel, grid, block, 0, s, x.t, x.g, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::hist: hipLaunchKernelGGL(bank_stream_hist_kernel, grid, block, 0, s, x.t, x.g, x.h, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::fx: hipLaunchKernelGGL(bank_stream_fx_kernel, grid, wave, 0, s, x.h, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::store: hipLaunchKernelGGL(bank_stream_store_kernel, grid, block, 0, s, x.t, x.g, x.h, x.s, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::store_fx: hipLaunchKernelGGL(bank_stream_store_fx_kernel, grid, wave, 0, s, x.h, x.s, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::sweep: hipLaunchKernelGGL(bank_stream_sweep_kernel, grid, block, 0, s, x.t, x.g, x.h, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::sweep_fx: hipLaunchKernelGGL(bank_stream_sweep_fx_kernel, grid, wave, 0, s, x.h, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::sweep_store: hipLaunchKernelGGL(bank_stream_sweep_store_kernel, grid, block, 0, s, x.t, x.g, x.h, x.s, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::sweep_store_fx: hipLaunchKernelGGL(bank_stream_sweep_store_fx_kernel, grid, wave, 0, s, x.h, x.s, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::leaf: hipLaunchKernelGGL(bank_stream_leaf_kernel, grid, block, 0, s, x.t, x.g, x.h, x.l, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::leaf_store: hipLaunchKernelGGL(bank_stream_leaf_store_kernel, grid, block, 0, s, x.t, x.g, x.h, x.s, x.l, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::track: hipLaunchKernelGGL(bank_stream_track_kernel, grid, block, 0, s, x.t, x.g, x.h, x.l, x.tr, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    case StreamKernel::track_store: hipLaunchKernelGGL(bank_stream_track_store_kernel, grid, block, 0, s, x.t, x.g, x.h, x.s, x.l, x.tr, x.a, x.p, x.n_rows, ctl_in, dev_in, idle_ms); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Partial-block exchange, one level of the voices' Sum2 trees (kernels.hpp ShardCombineArgs).  HBM-bound: 12 bytes per
// frame of a row; rows are contiguous and lanes run over frames, so every access is a full 256-byte line per wave.
__global__ void __launch_bounds__(256) shard_combine_kernel(ShardCombineArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t row = blockIdx.y;
    if (t >= a.len) return;
    const size_t e = (size_t)row * a.len + t;
    const float v = a.lo[e] + a.hi[e];
    if (a.dst_ws) { a.dst_ws[e] = v; return; }
    const uint32_t d = a.dst[row];
    if (d & 0x80000000u) a.rings[(size_t)(d & 0x7FFFFFFFu) * (a.ring_mask + 1) + ((a.ring_t0 + t) & a.ring_mask)] = v;
    else if (t >= a.out_skip) a.out[(size_t)d * a.out_stride + (t - a.out_skip)] = v;
}

hipError_t launch_shard_combine(const ShardCombineArgs &a, hipStream_t s) {
    if (a.n_rows == 0 || a.len == 0) return hipSuccess;
    const uint64_t bx = (a.len + 255) / 256;
    if (bx > 0x7FFFFFFFull) return hipErrorInvalidValue;
    for (uint32_t r0 = 0; r0 < a.n_rows; r0 += 65535u) {   // grid.y limit
        ShardCombineArgs c = a;
        c.n_rows = std::min<uint32_t>(a.n_rows - r0, 65535u);
        c.lo += (size_t)r0 * a.len;
        c.hi += (size_t)r0 * a.len;
        if (c.dst_ws) c.dst_ws += (size_t)r0 * a.len;
        if (c.dst) c.dst += r0;
        hipLaunchKernelGGL(shard_combine_kernel, dim3((uint32_t)bx, c.n_rows), dim3(256), 0, s, c);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------------
// Pieces of a voice -> the voice (kernels.hpp ChunkCombineArgs).  HBM-bound and tiny: 4 B x 2^C per output sample.
template <int C>
__global__ void __launch_bounds__(256) chunk_combine_kernel(ChunkCombineArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t voice = blockIdx.y;
    if (t >= a.n_times) return;
    float v[1 << C];
#pragma unroll
    for (int i = 0; i < (1 << C); ++i) v[i] = a.ws[(((size_t)voice << C) | (size_t)i) * a.n_times + t];
#pragma unroll
    for (int n = 1 << C; n > 1; n >>= 1)
#pragma unroll
        for (int i = 0; i < n / 2; ++i) v[i] = v[2 * i] + v[2 * i + 1];
    a.out[(size_t)a.rows[voice] * a.out_stride + t] = v[0];
}

hipError_t launch_chunk_combine(const ChunkCombineArgs &a, hipStream_t s) {
    if (a.n_voices == 0 || a.n_times == 0) return hipSuccess;
    if (a.log2_c < 1 || a.log2_c > 6 || a.n_voices > 65535u) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((a.n_times + 255) / 256), a.n_voices), block(256);
    switch (a.log2_c) {
    case 1: hipLaunchKernelGGL(chunk_combine_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(chunk_combine_kernel<2>, grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL(chunk_combine_kernel<3>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(chunk_combine_kernel<4>, grid, block, 0, s, a); break;
    case 5: hipLaunchKernelGGL(chunk_combine_kernel<5>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(chunk_combine_kernel<6>, grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
__global__ void pad_kernel(float *dst, uint64_t n, const float *src_last) {
    float v = src_last ? *src_last : 0.0f;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) dst[i] = v;
}

hipError_t launch_pad(float *dst, uint64_t n, const float *src_last, hipStream_t s) {
    if (n == 0) return hipSuccess;
    uint64_t blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(pad_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, dst, n, src_last);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Observed input ranges (kernels.hpp RangeArgs): per thread over a strided part of the row, then across the wave64 with
// lane shuffles, then across the block's four waves through LDS.  One partial result per block: no atomics on the mapped
// result.
__global__ __launch_bounds__(RANGE_THREADS) void input_range_kernel(RangeArgs a) {
    const uint32_t r = blockIdx.y;
    const float *p = a.row[r];
    const uint64_t n = a.len[r];
    float lo = __builtin_huge_valf(), hi = -__builtin_huge_valf();
    uint32_t fl = 0;
    const uint64_t step = (uint64_t)a.blocks * RANGE_THREADS;
    for (uint64_t i = (uint64_t)blockIdx.x * RANGE_THREADS + threadIdx.x; i < n; i += step) {
        const float v = p[i];
        if (v != v) fl |= RANGE_NAN;
        else if (v == __builtin_huge_valf()) fl |= RANGE_POS_INF;
        else if (v == -__builtin_huge_valf()) fl |= RANGE_NEG_INF;
        else { lo = fminf(lo, v); hi = fmaxf(hi, v); }
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
        fl |= __shfl_xor(fl, o, 64);
    }
    __shared__ float s_lo[RANGE_THREADS / 64], s_hi[RANGE_THREADS / 64];
    __shared__ uint32_t s_fl[RANGE_THREADS / 64];
    const uint32_t wave = threadIdx.x / 64;
    if ((threadIdx.x & 63u) == 0) { s_lo[wave] = lo; s_hi[wave] = hi; s_fl[wave] = fl; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < RANGE_THREADS / 64; ++w) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); fl |= s_fl[w]; }
        RangePart &o = a.out[(size_t)r * a.blocks + blockIdx.x];
        o.lo = lo;
        o.hi = hi;
        o.flags = fl;
        o.pad = 0;
    }
}

hipError_t launch_input_range(const RangeArgs &a, hipStream_t s) {
    if (a.n_rows == 0) return hipSuccess;
    if (a.n_rows > RANGE_MAX_ROWS || a.blocks == 0 || a.blocks > RANGE_MAX_BLOCKS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(input_range_kernel, dim3(a.blocks, a.n_rows), dim3(RANGE_THREADS), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------
// Track history (kernels.hpp TrackTailArgs): a pure streaming copy.  One wave per row, lanes over consecutive frames; the
// append is at most two contiguous spans of the ring (before and after its wrap).  A span whose source and destination are
// equally aligned moves as 16-byte loads and stores, with its unaligned head and tail element by element; otherwise, and
// for rows not supplied (+0.0), dword accesses, still 256 contiguous bytes per wave.
__device__ inline void track_span(float *dst, const float *src, uint64_t n, uint32_t lane) {
    const uint64_t mis = ((uintptr_t)dst & 15u) >> 2;                          // dst floats past a 16-byte boundary
    const bool vec = !src || (((uintptr_t)dst ^ (uintptr_t)src) & 15u) == 0;
    if (!vec) {
        for (uint64_t i = lane; i < n; i += 64) dst[i] = src[i];
        return;
    }
    const uint64_t head = mis ? (4 - mis < n ? 4 - mis : n) : 0;
    if (lane < head) dst[lane] = src ? src[lane] : 0.0f;
    const uint64_t nv = (n - head) >> 2;
    float4 *d4 = reinterpret_cast<float4 *>(dst + head);
    if (src) {
        const float4 *s4 = reinterpret_cast<const float4 *>(src + head);
        for (uint64_t i = lane; i < nv; i += 64) d4[i] = s4[i];
    } else {
        for (uint64_t i = lane; i < nv; i += 64) d4[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const uint64_t done = head + (nv << 2);
    if (lane < n - done) dst[done + lane] = src ? src[done + lane] : 0.0f;
}

__global__ __launch_bounds__(256) void track_tail_kernel(TrackTailArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t cap = a.mask + 1, p0 = a.first & a.mask;
    const uint64_t len0 = a.count < cap - p0 ? a.count : cap - p0;
    for (uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.rows; r += (uint64_t)gridDim.x * 4) {
        float *row = a.tail + r * cap;
        const float *src = r < a.src_rows ? a.src + r * a.src_stride + a.col0 : nullptr;
        track_span(row + p0, src, len0, lane);
        if (a.count > len0) track_span(row, src ? src + len0 : nullptr, a.count - len0, lane);
    }
}

hipError_t launch_track_tail(const TrackTailArgs &a, hipStream_t s) {
    if (a.rows == 0 || a.count == 0) return hipSuccess;
    if (a.count > a.mask + 1 || (a.src_rows && !a.src)) return hipErrorInvalidValue;
    uint64_t blocks = (a.rows + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(track_tail_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void track_window_kernel(TrackWindowArgs a) {
    const uint32_t r = blockIdx.y;
    float *dst = a.dst[r];
    const float *tail = a.tail[r], *call = a.call[r];
    const uint64_t len = a.back + a.n, t0 = a.idx - a.back;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < len; i += (uint64_t)gridDim.x * 256) {
        float v = 0.0f;
        if (i < a.back) { if (tail) v = tail[(t0 + i) & a.mask]; }
        else if (call) v = call[i - a.back];
        dst[i] = v;
    }
}

hipError_t launch_track_window(const TrackWindowArgs &a, hipStream_t s) {
    if (a.n_rows == 0 || a.back + a.n == 0) return hipSuccess;
    if (a.n_rows > TRACK_WINDOW_MAX_ROWS || a.back > a.idx) return hipErrorInvalidValue;
    uint64_t blocks = (a.back + a.n + 255) / 256;
    if (blocks > 64) blocks = 64;
    hipLaunchKernelGGL(track_window_kernel, dim3((uint32_t)blocks, a.n_rows), dim3(256), 0, s, a);
    return hipGetLastError();
}

// Kept delay lines (kernels.hpp RingMoveArgs): one wave per RING_MOVE_SEG-aligned segment of a descriptor's frames, lanes
// over consecutive frames (track_span: 16-byte accesses between equally aligned spans, heads and tails element by element).
__global__ __launch_bounds__(256) void ring_move_kernel(RingMoveArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (uint64_t)gridDim.x * 4;
    for (uint32_t di = blockIdx.y; di < a.n_desc; di += gridDim.y) {
        const RingMoveDesc d = a.desc[di];
        const uint64_t end = d.first + d.count;
        const float *src = a.src + (uint64_t)d.src_row * (a.src_mask + 1);
        float *dst = a.dst + (uint64_t)d.dst_row * (a.dst_mask + 1);
        for (uint64_t s0 = (d.first & ~(RING_MOVE_SEG - 1)) + wave * RING_MOVE_SEG; s0 < end; s0 += waves * RING_MOVE_SEG) {
            const uint64_t t0 = s0 > d.first ? s0 : d.first, t1 = s0 + RING_MOVE_SEG < end ? s0 + RING_MOVE_SEG : end;
            track_span(dst + (t0 & a.dst_mask), src + (t0 & a.src_mask), t1 - t0, lane);
        }
    }
}

hipError_t launch_ring_move(const RingMoveArgs &a, hipStream_t s) {
    if (a.n_desc == 0) return hipSuccess;
    if (!ring_move_in_bounds(a)) return hipErrorInvalidValue;
    uint64_t longest = 0;
    for (uint32_t i = 0; i < a.n_desc; ++i) longest = std::max(longest, a.host_desc[i].count);
    if (longest == 0) return hipSuccess;
    const uint64_t segs = longest / RING_MOVE_SEG + 2;   // (a span that starts inside a segment touches one more)
    const uint32_t bx = (uint32_t)std::min<uint64_t>((segs + 3) / 4, 64);
    hipLaunchKernelGGL(ring_move_kernel, dim3(bx, std::min<uint32_t>(a.n_desc, 65535u)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace fr
