// callplan_tests.cpp -- the per-call rule (csrc/callplan.hpp) over a pinned table: ring capacity, the call's windows, the
// exchange tiles and the stage launch form.  The expected values were worked out by hand from the arithmetic as it stood
// inline in the engine's execute(), so a change of any of them shows up here.
//
// Build: g++ -std=c++17 -O1 -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -o callplan_tests callplan_tests.cpp
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../libfriendship_amd/csrc/callplan.hpp"

using namespace fr;

namespace {

int g_passed = 0, g_failed = 0;
void expect(bool ok, const char *what) {
    if (ok) { ++g_passed; return; }
    ++g_failed;
    std::printf("FAILED: %s\n", what);
}
#define EXPECT(cond) expect((cond), #cond)

using Tiles = std::vector<std::pair<uint64_t, uint64_t>>;   // (offset in the window, frames)
Tiles tiles(uint64_t xlen, bool serial, uint32_t max_tiles = 4, uint32_t min_tile = 1024) {
    const ExchangeTiles t = exchange_tiles(xlen, serial, max_tiles, min_tile);
    Tiles v;
    for (uint32_t i = 0; i < t.count; ++i) v.push_back({t.offset(i), t.frames(i)});
    return v;
}

// A plan with rings, `n_levels` levels and a fused form.
StagedPlan ring_plan(uint64_t lmax, size_t n_levels = 10, uint64_t fused_stride = 300, uint64_t fused_max_frames = 300) {
    StagedPlan sp;
    sp.n_rings = 1;
    sp.lmax = lmax;
    sp.progs.resize(n_levels + 1);
    for (uint32_t l = 0; l <= n_levels; ++l) sp.level_first.push_back(l);
    sp.fused_first = (uint32_t)n_levels;
    sp.fused_count = 1;
    sp.fused_stride = fused_stride;
    sp.fused_max_frames = fused_max_frames;
    return sp;
}
StagedPlan feedback_plan(uint64_t lmax) {
    StagedPlan sp = ring_plan(lmax);
    sp.feedback = true;
    return sp;
}
CallIn call(uint64_t idx, uint64_t n_times, bool rings_valid, bool keep_on = false, bool repair_replay = false) {
    return CallIn{idx, n_times, rings_valid, keep_on, repair_replay};
}
StageForm form_of(const StagedPlan &sp, const CallIn &c, uint64_t min_stride = STRIDED_MIN_STRIDE, bool strided_ok = true) {
    return stage_form(sp, c, call_windows(sp, c), min_stride, strided_ok);
}

void exchange_tile_table() {
    EXPECT((tiles(4800, false) == Tiles{{0, 1216}, {1216, 1216}, {2432, 1216}, {3648, 1152}}));
    EXPECT((tiles(1000, false) == Tiles{{0, 1000}}));
    EXPECT((tiles(300, false, 4, 64) == Tiles{{0, 128}, {128, 128}, {256, 44}}));
    EXPECT((tiles(4800, exchange_serial(true, true, true)) == Tiles{{0, 4800}}));      // the serial flag
    EXPECT((tiles(4800, exchange_serial(false, false, false)) == Tiles{{0, 4800}}));   // host-callback transport, tiles not asked for
    EXPECT(!exchange_serial(false, true, false));                                      // RCCL tiles by default
    EXPECT(!exchange_serial(false, false, true));                                      // ... and any transport when asked
    EXPECT((tiles(4800, false, 2) == Tiles{{0, 2432}, {2432, 2368}}));
    EXPECT((tiles(2, false) == Tiles{{0, 2}}));
}

void ring_capacity_table() {
    EXPECT(ring_capacity(ring_plan(79), 333) == 1024);
    EXPECT(ring_capacity(ring_plan(7200), 4800) == 16384);
    EXPECT(ring_capacity(feedback_plan(300), 64) == 32768);   // room for FB_CHUNK
    EXPECT(ring_capacity(ring_plan(1000), 24) == 1024);
    EXPECT(ring_capacity(ring_plan(1000), 25) == 2048);
    EXPECT(FB_CHUNK == 16384 && FB_MAX_REPLAY == (1ull << 28));
}

void window_table() {
    const StagedPlan sp = ring_plan(79);
    CallWindows w = call_windows(sp, call(1000, 333, true));
    EXPECT(w.w0 == 1000 && w.w_len == 333 && w.rings_current && !w.fb_replay);
    w = call_windows(sp, call(1000, 333, false));
    EXPECT(w.w0 == 921 && w.w_len == 412 && !w.rings_current);
    w = call_windows(sp, call(50, 333, false));   // clamped at 0
    EXPECT(w.w0 == 0 && w.w_len == 383 && !w.rings_current);
    w = call_windows(sp, call(1000, 333, false, true));   // kept rings: current whatever stage_valid said
    EXPECT(w.w0 == 1000 && w.w_len == 333 && w.rings_current && !w.fb_replay);
    StagedPlan none;   // no rings: nothing is ever "current", the window is the call
    w = call_windows(none, call(1000, 333, true));
    EXPECT(w.w0 == 1000 && w.w_len == 333 && !w.rings_current);

    const StagedPlan fb = feedback_plan(300);
    w = call_windows(fb, call(5000, 64, false));
    EXPECT(w.fb_replay && w.w0 == 5000 && w.w_len == 64 && !w.rings_current);
    w = call_windows(fb, call(0, 64, false));
    EXPECT(!w.fb_replay && w.w0 == 0 && w.w_len == 64);
    w = call_windows(fb, call(5000, 64, true));
    EXPECT(!w.fb_replay && w.rings_current);
    w = call_windows(fb, call(5000, 64, false, true));   // kept rings: the repair replays, not the call
    EXPECT(!w.fb_replay && w.rings_current);
    w = call_windows(fb, call(1ull << 28, 64, false));   // the last frame a replay reaches
    EXPECT(w.fb_replay);
    for (bool keep : {false, true}) {   // (with kept rings it is the repair's replay that is refused)
        bool refused = false;
        try {
            call_windows(fb, call((1ull << 28) + 1, 64, false, keep, keep));
        } catch (const Error &e) {
            refused = e.code == FR_ERR_UNSUPPORTED &&
                      !std::strcmp(e.what(), "a feedback loop's state at frame 268435457 would take replaying more than 2^28 frames");
        }
        EXPECT(refused);
    }

    // the exchange window: the call's frames, or the staged window when a split voice feeds a ring
    StagedPlan xs = ring_plan(79);
    xs.split.push_back(SplitVoice{0, false, 0});
    w = call_windows(xs, call(1000, 333, false));
    EXPECT(w.x0 == 1000 && w.xlen == 333);
    xs.split.push_back(SplitVoice{1, true, 0});
    w = call_windows(xs, call(1000, 333, false));
    EXPECT(w.x0 == 921 && w.xlen == 412);
    w = call_windows(xs, call(1000, 333, true));
    EXPECT(w.x0 == 1000 && w.xlen == 333);
}

void stage_form_table() {
    const StagedPlan sp = ring_plan(7200);   // fused_stride 300, fused_max_frames 300, 10 levels
    StageForm f = form_of(sp, call(4800, 517, true));
    EXPECT(f.kind == StageForm::strided && f.sub_windows == 2);
    f = form_of(sp, call(4800, 2317, true));
    EXPECT(f.kind == StageForm::strided && f.sub_windows == 8);
    f = form_of(sp, call(4800, 2401, true));   // 9 strides: no longer one launch; 9 sub-windows < 10 levels
    EXPECT(f.kind == StageForm::fused && f.sub_windows == 9 && f.fused_step == 300);
    f = form_of(ring_plan(7200, 9), call(4800, 2401, true));   // ... but not < 9 levels
    EXPECT(f.kind == StageForm::levels);
    f = form_of(sp, call(4800, 517, true), STRIDED_MIN_STRIDE, false);   // FR_STAGE_STRIDED=0
    EXPECT(f.kind == StageForm::fused && f.sub_windows == 2 && f.fused_step == 300);
    EXPECT(STRIDED_MIN_STRIDE == 256);
    f = form_of(ring_plan(7200, 10, 255), call(4800, 517, true));   // 3 strides of 255: too short a stride for the engine
    EXPECT(f.kind == StageForm::fused && f.sub_windows == 2);
    f = form_of(ring_plan(7200, 10, 255), call(4800, 517, true), 16);   // (the test-side simulator's min_stride takes it)
    EXPECT(f.kind == StageForm::strided && f.sub_windows == 3);
    f = form_of(sp, call(4800, 300, true));   // one stride: a plain fused launch
    EXPECT(f.kind == StageForm::fused && f.sub_windows == 1);
    for (uint64_t T : {64u, 517u, 2401u}) {
        const CallIn c = call(20000, T, false);   // rings not current: levels over the look-back window
        const CallWindows w = call_windows(sp, c);
        EXPECT(form_of(sp, c).kind == StageForm::levels && w.w0 == 12800 && w.w_len == 7200 + T);
        EXPECT(form_of(feedback_plan(300), call(20000, T, false)).kind == StageForm::feedback);
        EXPECT(form_of(feedback_plan(300), call(20000, T, true)).kind == StageForm::feedback);
    }
    StagedPlan no_fused = ring_plan(79);
    no_fused.fused_count = 0;
    EXPECT(form_of(no_fused, call(4800, 517, true)).kind == StageForm::levels);
    StagedPlan banks_only;
    EXPECT(form_of(banks_only, call(0, 64, false)).kind == StageForm::none);
}

}  // namespace

int main() {
    exchange_tile_table();
    ring_capacity_table();
    window_table();
    stage_form_table();
    std::printf("%d passed; %d failed\n", g_passed, g_failed);
    return g_failed ? 1 : 0;
}
