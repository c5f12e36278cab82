"""Every launch form a track voice can take, and the smallest GPU case that reaches each (plain data: importable
without a GPU).

Track voices (synth.track_tree: every partial's w and amp read from input rows, fr_set_track_inputs) always run the generated
kernel with NT > 0: the row values of an 8-leaf group are requested one group ahead, slots at or beyond the call's limit read
+0, lanes past the call's end re-read its last frame, plan_bank cuts voices into pieces by rules of its own (a target of 16384
workgroups; pieces of 256 partials on calls of at most 128 frames), and with FR_TRACK_HISTORY the same kernel is aimed at
spans of the history ring.  A key is what fr_plan_json's "bank_launches" reports as "variant".  tests/cpp/bankplan_sweep.cpp
--tracks prints every key the rule can produce for a group with tracks; tests/test_track_variants.py checks on the CPU that
this table has exactly those keys and that each case's shape and options reach its key on both call lengths.
tests/test_hip_track_matrix.py runs every case on the GPU against the dense reference (bank_reference.render_track_bank).

A case: V voices of P partials in ONE group (no leaf constant differs between track voices), two call lengths T (the ramp and
the hostile call) and T2 (a later call that reuses the pieces' workspace; the same number of 64-frame tiles as T wherever a
FR_JIT_CHUNK_TARGET decides the piece count, so that both calls reach the key), the per-renderer options, the entry point
("dense": fill_buffer_dense, "csr": fill_buffer, "device_dense": fill_buffer_device_dense), and `xcd`: whether the first
call's workgroup count is a multiple of 8 (the kernels then remap blocks to XCD-contiguous ranges).  `pieces_log2` and
`groups` (8-leaf groups per wave: P / 2^pieces_log2 / 4 waves / 8, whole voices per wave: P / 8) follow from the key; a case
with groups >= 2 runs the one-group-ahead reload (`g + 1 < ngroups`), groups == 1 only the first request.  `fresh`: the case
also runs on a renderer without the priming call, so that the slot limit n_slots * T falls inside a voice.

FR_JIT_CHUNK_TARGET = workgroups-per-voice-row << k stops the rule at exactly 2^k pieces: V voices x 5 tiles at T = 300.
"""


def _target(V, T, k):
    return {"FR_JIT_CHUNK_TARGET": str((V * -(-T // 64)) << k)}


def _case(name, key, V, P, T, T2, options=None, entry="dense", xcd=False, fresh=False):
    k = int(key.split("pieces")[1]) if "pieces" in key else 0
    groups = P // 8 if key == "jit_bank_multi" else (P >> k) // 32
    return {"name": name, "key": key, "V": V, "P": P, "T": T, "T2": T2, "options": dict(options or {}), "entry": entry, "xcd": xcd,
            "fresh": fresh, "pieces_log2": k, "groups": groups}


CASES = [
    # one piece per voice: 25 workgroups, two groups per wave
    _case("whole voices", "jit_bank", 5, 64, 300, 270, {"FR_JIT_CHUNK_TARGET": "1"}),
    # 2^k pieces of 64 partials (two groups per wave; the second is the prefetched one) + chunk_combine_kernel<k>;
    # 30 workgroups: not a multiple of 8; the others are
    _case("pieces1", "jit_bank/pieces1", 3, 128, 300, 270, _target(3, 300, 1), entry="csr"),
    _case("pieces2", "jit_bank/pieces2", 4, 256, 300, 270, _target(4, 300, 2), entry="device_dense", xcd=True),
    _case("pieces3", "jit_bank/pieces3", 4, 512, 300, 270, _target(4, 300, 3), xcd=True),
    _case("pieces4", "jit_bank/pieces4", 4, 1024, 300, 270, _target(4, 300, 4), entry="csr", xcd=True),
    _case("pieces5", "jit_bank/pieces5", 4, 2048, 300, 270, _target(4, 300, 5), entry="device_dense", xcd=True),
    _case("pieces6", "jit_bank/pieces6", 4, 4096, 300, 270, _target(4, 300, 6), xcd=True),
    # pieces of 32 partials, the smallest the rule makes: ONE group per wave, the reload never runs
    _case("pieces6 of one group", "jit_bank/pieces6", 4, 2048, 300, 270, {"FR_JIT_CHUNK_TARGET": "65536"}, entry="device_dense", xcd=True),
    # the default target (16384 workgroups for tracks, 1024 otherwise: 20 << 3 = 160 < 1024 too, so a case under the default
    # cannot tell the two at this size; the sweep does): cut down to the 32-partial floor
    _case("default target", "jit_bank/pieces3", 4, 256, 300, 270, xcd=True),
    # calls of at most 128 frames, voices of 256 partials and more: pieces of 256 partials whatever the target says --
    # 2^(10 - 8) pieces of a 1024-partial voice (the target alone would give 2^5), and whole 256-partial voices (2^3)
    _case("short call rule", "jit_bank/pieces2", 4, 1024, 100, 70, xcd=True),
    _case("short call rule, whole voices", "jit_bank", 5, 256, 100, 70, entry="device_dense"),
    # the slot limit mid-voice and mid-group: no priming call, limit 4 x 301 = 1204 = the amp slot of partial 89 of voice 2
    _case("fresh renderer", "jit_bank/pieces2", 4, 256, 301, 270, _target(4, 301, 2), xcd=True, fresh=True),
    # many small voices, whole voices per wave (1030 is no multiple of 4: the last workgroup's waves partly empty)
    _case("whole voices per wave", "jit_bank_multi", 1030, 32, 200, 250, entry="device_dense", xcd=True),
]

# Launch forms of compiled voices that a track group never takes, and why: none.  jit_bank_multi is reachable -- every generated
# module has the entry, so the engine sets BankCall::jit_multi for track groups as for any compiled group (engine.cpp
# `bs.jit && bs.jit->fn_multi`).
UNREACHABLE = {}

# Families whose kernels remap workgroups when their count is a multiple of 8: a case on either side.
XCD_FAMILIES = ("jit_bank",)

# ---- ring spans (FR_TRACK_HISTORY) --------------------------------------------------------------------------------------
# Voices out_v = Delay(voice_v, d): the voices render into delay rings of max(1024, pow2 >= d + n) frames.  A call longer
# than any before grows those rings, which loses them: the voices' window is then [idx - d, idx + n), and its part before idx
# is rendered from the track history ring (H2 = 64 floats per row for every H <= 64, the smallest the option makes), one
# launch per span, cut where that ring wraps (frame & 63 == 0), then the call's own frames.  H = 1 is the smallest history the
# option takes; its window is one frame and cannot straddle, so the straddling sequences use H = d = 40 on the same 64-frame
# ring.  `calls`: (idx, frames, bank launches expected: spans + 1).  The first call primes every row (3 x 200 >= 193).
SPAN_V, SPAN_P = 3, 32
SPAN_CASES = [
    # [317, 357) straddles 320: spans [317, 320) (3 frames: one partial tile, 61 clamped lanes) and [320, 357), then the call
    {"name": "straddles the wrap", "H": 40, "d": 40, "calls": [(0, 200, 1), (200, 157, 1), (357, 1000, 3), (1357, 77, 1)]},
    # [320, 360) starts on the wrap: one span
    {"name": "starts on the wrap", "H": 40, "d": 40, "calls": [(0, 200, 1), (200, 160, 1), (360, 1000, 2), (1360, 77, 1)]},
    # [383, 384) ends on the wrap, the smallest history; then a seek (the history reads +0; [4999, 5000) is one span)
    {"name": "smallest history", "H": 1, "d": 1, "calls": [(0, 200, 1), (200, 184, 1), (384, 1100, 2), (5000, 130, 2)]},
    # [217, 257) straddles 256 one frame before its end (spans of 39 and 1 frames); a second growth (2048 -> 4096 frames per
    # delay ring) whose window [1217, 1257) starts one frame after a wrap: one span that is not aligned to the ring
    {"name": "second growth", "H": 40, "d": 40, "calls": [(0, 200, 1), (200, 57, 1), (257, 1000, 3), (1257, 2100, 2)]},
]
