"""Every kernel instance the bank launch rule can pick, and the smallest GPU case that reaches each (plain data: importable
without a GPU).

A key is what fr_plan_json's "bank_launches" reports as "variant" (csrc/bankplan.hpp bank_variant).  tests/cpp/bankplan_sweep.cpp
sweeps the rule and prints every key it can produce; tests/test_bank_variants.py checks on the CPU that this table has
exactly those keys, that each case's shape and options reach its key, and that no key listed in UNREACHABLE appears.
tests/test_hip_bank_matrix.py runs every case on the GPU against the dense reference (tests/bank_reference.py).

A case: the group kind ("balanced": power-of-two template voices; "general": a partial count that is not a power of two;
"jit": template voices through the generated kernel, FR_BANK_TEMPLATE=0), V voices of P partials, two call lengths T and T2
(the first call and a hostile row have T frames, a later call T2), the per-renderer options, and the entry point ("host":
fill_buffer, whose results of 256 KB and more stream rows through row flags; "device": fill_buffer_device, never flags).
`xcd`: whether the first call's workgroup count is a multiple of 8 (the kernels then remap blocks to XCD-contiguous ranges).
Generated kernels compile the two silent voices of the GPU test (amplitudes all literal zeros) as groups of their own: for
"jit" cases the key and `xcd` are those of the main group, V - 2 voices.
"""

# (FR_BANK_SHORT=0 keeps few-pair shapes off the short-call kernel; FR_BANK_LEAF=0 selects the product-form leaves, MODE 0)
_NOSHORT = {"FR_BANK_SHORT": "0"}
_LEAF0 = {"FR_BANK_LEAF": "0"}


def _case(key, kind, V, P, T, T2, options=None, entry="device", xcd=False):
    return {"key": key, "kind": kind, "V": V, "P": P, "T": T, "T2": T2, "options": dict(options or {}), "entry": entry, "xcd": xcd}


CASES = [
    # time-major kernel, one chunk per voice, FMA-form leaves (MODE 1)
    _case("bank_kernel<F1,M1,NW4>", "balanced", 5, 32, 300, 200),
    _case("bank_kernel<F1,M1,NW8>", "balanced", 6, 256, 300, 260),
    _case("bank_kernel<F1,M1,NW1>", "balanced", 1100, 32, 300, 270, {"FR_BANK_MULTI": "0"}),
    _case("bank_kernel<F2,M1,NW4>", "balanced", 5, 32, 300, 200, {"FR_BANK_F": "2"}),
    _case("bank_kernel<F2,M1,NW8>", "balanced", 6, 64, 300, 260, {"FR_BANK_F": "2"}),
    _case("bank_kernel<F4,M1,NW4>", "balanced", 5, 32, 600, 520, {"FR_BANK_F": "4"}),
    _case("bank_kernel<F4,M1,NW8>", "balanced", 6, 64, 600, 520, {"FR_BANK_F": "4"}),
    # ... publishing row flags to the streamed host output (256 KB of output and more)
    _case("bank_kernel<F1,M1,NW4,flags>", "balanced", 16, 32, 4200, 4500, entry="host", xcd=True),
    _case("bank_kernel<F1,M1,NW8,flags>", "balanced", 16, 64, 4200, 4500, entry="host", xcd=True),
    _case("bank_kernel<F2,M1,NW4,flags>", "balanced", 17, 32, 4200, 4500, {"FR_BANK_F": "2"}, entry="host"),
    _case("bank_kernel<F2,M1,NW8,flags>", "balanced", 16, 64, 4200, 4500, {"FR_BANK_F": "2"}, entry="host", xcd=True),
    _case("bank_kernel<F4,M1,NW4,flags>", "balanced", 16, 32, 4200, 4500, {"FR_BANK_F": "4"}, entry="host", xcd=True),
    _case("bank_kernel<F4,M1,NW8,flags>", "balanced", 16, 64, 4200, 4500, {"FR_BANK_F": "4"}, entry="host", xcd=True),
    # product-form leaves (MODE 0)
    _case("bank_kernel<F1,M0,NW4>", "balanced", 5, 32, 300, 200, _LEAF0),
    _case("bank_kernel<F1,M0,NW8>", "balanced", 8, 256, 300, 260, _LEAF0, xcd=True),
    _case("bank_kernel<F2,M0,NW4>", "balanced", 5, 32, 300, 200, {**_LEAF0, "FR_BANK_F": "2"}),
    _case("bank_kernel<F2,M0,NW8>", "balanced", 6, 64, 300, 260, {**_LEAF0, "FR_BANK_F": "2"}),
    _case("bank_kernel<F4,M0,NW4>", "balanced", 5, 32, 600, 520, {**_LEAF0, "FR_BANK_F": "4"}),
    _case("bank_kernel<F4,M0,NW8>", "balanced", 6, 64, 600, 520, {**_LEAF0, "FR_BANK_F": "4"}),
    # voices cut into chunks, then bank_combine_kernel: few big voices on a long call (>= 512 frames), or more than one
    # workgroup's partials (2^14 with 8 waves)
    _case("bank_kernel<F1,M1,NW4>+combine", "balanced", 4, 1024, 600, 530, _NOSHORT, xcd=True),
    _case("bank_kernel<F1,M0,NW4>+combine", "balanced", 4, 1024, 600, 530, {**_NOSHORT, **_LEAF0}, xcd=True),
    _case("bank_kernel<F1,M1,NW8>+combine", "balanced", 4, 32768, 130, 70, _NOSHORT, xcd=True),
    _case("bank_kernel<F1,M0,NW8>+combine", "balanced", 4, 32768, 130, 70, {**_NOSHORT, **_LEAF0}, xcd=True),
    _case("bank_kernel<F2,M1,NW8>+combine", "balanced", 4, 32768, 130, 70, {**_NOSHORT, "FR_BANK_F": "2"}, xcd=True),
    _case("bank_kernel<F2,M0,NW8>+combine", "balanced", 4, 32768, 130, 70, {**_NOSHORT, **_LEAF0, "FR_BANK_F": "2"}, xcd=True),
    _case("bank_kernel<F4,M1,NW8>+combine", "balanced", 4, 32768, 130, 70, {**_NOSHORT, "FR_BANK_F": "4"}, xcd=True),
    _case("bank_kernel<F4,M0,NW8>+combine", "balanced", 4, 32768, 130, 70, {**_NOSHORT, **_LEAF0, "FR_BANK_F": "4"}, xcd=True),
    # many small voices, whole voices per wave (voice counts not a multiple of 4 x voices_per_wave)
    _case("bank_multi_kernel<F1,M1>", "balanced", 301, 32, 1000, 1010, xcd=True),
    _case("bank_multi_kernel<F1,M0>", "balanced", 301, 32, 1000, 1010, _LEAF0, xcd=True),
    _case("bank_multi_kernel<F2,M1>", "balanced", 1900, 32, 1100, 1030),
    _case("bank_multi_kernel<F2,M0>", "balanced", 521, 32, 1100, 1030, _LEAF0),
    # short calls: lanes over frames, parameters staged in LDS; whole voices, or chunks added up in the launch (tickets)
    _case("bank_short_kernel<NW16>", "balanced", 4, 512, 200, 130, xcd=True),
    _case("bank_short_kernel<NW8>", "balanced", 4, 512, 200, 130, {"FR_SHORT_NW": "8"}, xcd=True),
    _case("bank_short_kernel<NW4>", "balanced", 4, 512, 200, 130, {"FR_SHORT_NW": "4"}, xcd=True),
    _case("bank_short_kernel<NW16>+tickets", "balanced", 4, 4096, 200, 130, xcd=True),
    _case("bank_short_kernel<NW8>+tickets", "balanced", 4, 4096, 200, 130, {"FR_SHORT_NW": "8", "FR_SHORT_WGS": "64"}, xcd=True),
    _case("bank_short_kernel<NW4>+tickets", "balanced", 4, 4096, 200, 130, {"FR_SHORT_NW": "4"}, xcd=True),
    # calls of at most 2 frames: lanes over partials, 256 per workgroup
    _case("bank_small_kernel", "balanced", 5, 256, 2, 1),
    _case("bank_small_kernel+combine", "balanced", 5, 1024, 2, 1, _NOSHORT),
    # voices that are not power-of-two trees: the schedule kernels
    _case("gbank_kernel", "general", 5, 100, 300, 200),
    _case("gbank_multi_kernel", "general", 301, 24, 1000, 1010, xcd=True),
    # generated kernels (hipRTC): one piece per voice, 2^k pieces + chunk_combine_kernel<k>, many small voices
    _case("jit_bank", "jit", 5, 64, 300, 270, {"FR_BANK_TEMPLATE": "0", "FR_JIT_CHUNK_TARGET": "1"}),
    _case("jit_bank/pieces1", "jit", 4, 64, 300, 270, {"FR_BANK_TEMPLATE": "0", "FR_JIT_CHUNK_TARGET": "65536"}),
    _case("jit_bank/pieces2", "jit", 4, 128, 300, 270, {"FR_BANK_TEMPLATE": "0", "FR_JIT_CHUNK_TARGET": "65536"}, xcd=True),
    _case("jit_bank/pieces3", "jit", 4, 256, 300, 270, {"FR_BANK_TEMPLATE": "0", "FR_JIT_CHUNK_TARGET": "65536"}, xcd=True),
    _case("jit_bank/pieces4", "jit", 4, 512, 300, 270, {"FR_BANK_TEMPLATE": "0", "FR_JIT_CHUNK_TARGET": "65536"}, xcd=True),
    _case("jit_bank/pieces5", "jit", 4, 1024, 300, 270, {"FR_BANK_TEMPLATE": "0", "FR_JIT_CHUNK_TARGET": "65536"}, xcd=True),
    _case("jit_bank/pieces6", "jit", 4, 2048, 300, 270, {"FR_BANK_TEMPLATE": "0", "FR_JIT_CHUNK_TARGET": "65536"}, xcd=True),
    _case("jit_bank_multi", "jit", 301, 32, 1000, 1010, {"FR_BANK_TEMPLATE": "0"}, xcd=True),
]

# Instantiations compiled into the library that the rule never picks (kernels.hip launch_bank / launch_bank_f), and why.
UNREACHABLE = {
    "bank_kernel<F1,M2,NW4>": "MODE 2 (no zero-sign repair) is diagnostic only: BankTuning::leaf_variant is 0 or 1",
    "bank_kernel<F2,M2,NW4>": "MODE 2 (no zero-sign repair) is diagnostic only: BankTuning::leaf_variant is 0 or 1",
    "bank_kernel<F4,M2,NW4>": "MODE 2 (no zero-sign repair) is diagnostic only: BankTuning::leaf_variant is 0 or 1",
    "bank_multi_kernel<F1,M2>": "MODE 2 (no zero-sign repair) is diagnostic only: BankTuning::leaf_variant is 0 or 1",
    "bank_multi_kernel<F2,M2>": "MODE 2 (no zero-sign repair) is diagnostic only: BankTuning::leaf_variant is 0 or 1",
    "bank_kernel<F1,M1,NW2>": "nothing in bank_shape or plan_bank sets 2 waves per workgroup",
    "bank_kernel<F2,M1,NW2>": "nothing in bank_shape or plan_bank sets 2 waves per workgroup",
    "bank_kernel<F4,M1,NW2>": "nothing in bank_shape or plan_bank sets 2 waves per workgroup",
    "bank_kernel<F2,M1,NW1>": "plan_bank picks 1 wave per workgroup only with one frame per lane",
    "bank_kernel<F4,M1,NW1>": "plan_bank picks 1 wave per workgroup only with one frame per lane",
}

# Families whose kernels remap workgroups when their count is a multiple of 8: each has a case on either side.
XCD_FAMILIES = ("bank_kernel<", "bank_multi_kernel<", "gbank", "jit_bank")
