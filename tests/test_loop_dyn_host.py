"""FR_LOOP_DYN's plain logic (csrc/stage.hpp sweep_bound, csrc/callplan.hpp loop_sweep) as a stand-alone C++ program on the CPU,
built with AddressSanitizer and UndefinedBehaviorSanitizer: tests/cpp/loopdyn_tests.cpp checks W over mixed constant and signal
reads on hand-built plans, the rule's answer and every reason for both forms and every edge of the wave and of the cap, what
loop_tile answers a sweep plan, and a plain-loop model of the sweep form in which, for random amounts inside their proven
ranges, no frame of a sweep reads a frame of the same sweep."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "loopdyn_tests.cpp")
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("callplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp")]
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "loopdyn_tests")


def test_loop_dyn_rule_under_sanitizers():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in [SRC] + DEPS):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        # (the rule's header includes the plan's types, which name HIP's: its headers, no HIP library)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", BIN, SRC], check=True)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
