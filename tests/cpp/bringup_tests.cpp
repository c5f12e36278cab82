// bringup_tests.cpp -- a call of ZERO own frames (libfriendship_amd/csrc/callplan.hpp bring_up_form with call_windows): what a
// stream that continues the input store (FR_STREAM_STORE) has the engine do before its resident launch starts at idx.  Every
// early-out of the rule over hand-built plans: a call with frames of its own, a plan without programs, a feedback plan (its
// replay), rings that are current, FR_RING_KEEP (the repair), and an empty window.  Stand-alone: built and run on the CPU with
// -fsanitize=address,undefined by tests/test_stream_store_host.py.
#include <cstdio>

#include "../../libfriendship_amd/csrc/callplan.hpp"

using namespace fr;

static int passed = 0, failed = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (cond) ++passed;                                                         \
        else { ++failed; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// A plan with one ring, `levels` levels of one program each and a fused form.
static StagedPlan ring_plan(uint64_t lmax, uint32_t levels = 3) {
    StagedPlan sp;
    sp.n_rings = 1;
    sp.lmax = lmax;
    sp.progs.resize(levels + 1);
    for (uint32_t l = 0; l <= levels; ++l) sp.level_first.push_back(l);
    sp.fused_first = levels;
    sp.fused_count = 1;
    sp.fused_stride = sp.fused_max_frames = 300;
    return sp;
}
static CallIn zero(uint64_t idx, bool rings_valid, bool keep_on = false) { return CallIn{idx, 0, rings_valid, keep_on, false}; }

int main() {
    const StagedPlan sp = ring_plan(100);
    {   // rings not current: the look-back window in front of idx, level by level, and no frame of its own
        const CallIn c = zero(295, false);
        const CallWindows w = call_windows(sp, c);
        CHECK(w.w0 == 195 && w.w_len == 100 && !w.rings_current && !w.fb_replay);
        CHECK(bring_up_form(sp, c, w).kind == StageForm::levels);
        CHECK(stage_form(sp, c, w, STRIDED_MIN_STRIDE, true).kind == StageForm::none);     // (the per-call rule knows no call without frames)
    }
    {   // ... cut at frame 0
        const CallIn c = zero(40, false);
        const CallWindows w = call_windows(sp, c);
        CHECK(w.w0 == 0 && w.w_len == 40 && bring_up_form(sp, c, w).kind == StageForm::levels);
    }
    {   // 1. a call with frames of its own is not a bring-up
        CallIn c = zero(295, false);
        c.n_times = 64;
        CHECK(bring_up_form(sp, c, call_windows(sp, c)).kind == StageForm::none);
    }
    {   // 2. no programs: the ring-bound banks alone render the window (the engine's phase), no stage launch
        StagedPlan banks_only = sp;
        banks_only.progs.clear();
        const CallIn c = zero(295, false);
        const CallWindows w = call_windows(banks_only, c);
        CHECK(w.w_len == 100 && bring_up_form(banks_only, c, w).kind == StageForm::none);
    }
    {   // 3. a feedback plan replays from frame 0; its own window is empty
        StagedPlan fb = sp;
        fb.feedback = true;
        const CallIn c = zero(295, false);
        const CallWindows w = call_windows(fb, c);
        CHECK(w.fb_replay && w.w0 == 295 && w.w_len == 0 && bring_up_form(fb, c, w).kind == StageForm::none);
        const CallIn at0 = zero(0, false);
        CHECK(!call_windows(fb, at0).fb_replay);                                             // nothing before frame 0
        const CallIn cur = zero(295, true);
        CHECK(!call_windows(fb, cur).fb_replay);                                             // steady: nothing
    }
    {   // 4. rings current -- the call would be steady -- and FR_RING_KEEP, whose repair has brought them up: nothing
        const CallIn steady = zero(295, true), kept = zero(295, false, true);
        for (const CallIn &c : {steady, kept}) {
            const CallWindows w = call_windows(sp, c);
            CHECK(w.rings_current && w.w0 == 295 && w.w_len == 0 && bring_up_form(sp, c, w).kind == StageForm::none);
        }
    }
    {   // 5. an empty window: idx 0, and a plan without rings (programs that read the current frame only)
        const CallIn c = zero(0, false);
        const CallWindows w = call_windows(sp, c);
        CHECK(w.w_len == 0 && bring_up_form(sp, c, w).kind == StageForm::none);
        StagedPlan flat = sp;
        flat.n_rings = 0;
        flat.lmax = 0;
        const CallIn d = zero(295, false);
        const CallWindows v = call_windows(flat, d);
        CHECK(v.w0 == 295 && v.w_len == 0 && bring_up_form(flat, d, v).kind == StageForm::none);
    }
    {   // the rings such a call sizes are a block's (the engine asks ring_capacity with the frames the launch will render)
        CHECK(ring_capacity(sp, 64) == 1024 && ring_capacity(ring_plan(1000), 64) == 2048);
    }
    std::printf("%d passed; %d failed\n", passed, failed);
    return failed ? 1 : 0;
}
