"""FR_STREAM_SWEEP on the host (csrc/streamplan.hpp, csrc/kernels.hpp) as a stand-alone C++ program on the CPU, built with
AddressSanitizer and UndefinedBehaviorSanitizer: tests/cpp/streamsweep_tests.cpp checks the width and slot-marking helpers on
hand-built programs, the serving rule and the launch rule on hand-built plans, the form and the launch check of the four sweep
kernels, and a plain-loop model of the sweep walk against a frame-by-frame evaluation of the same instructions, bit for bit, over
hundreds of consecutive blocks of random length."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "streamsweep_tests.cpp")
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("streamplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp")] + [
    os.path.join(ROOT, "tests", "cpp", "streamplans.hpp")]
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "streamsweep_tests")


def test_stream_sweep_helpers_rule_check_and_walk_under_sanitizers():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in [SRC] + DEPS):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        # (the rule's header includes the plan's types, which name HIP's: its headers, no HIP library)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", BIN, SRC], check=True)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
