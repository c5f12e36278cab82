"""FR_STREAM_TAPS on the host (csrc/streamplan.hpp) as a stand-alone C++ program on the CPU, built with AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/streamtaps_tests.cpp checks the serving rule on hand-built plans without feedback and
without a fused form (the run form in level order, a reader that follows its storer, two storers that make a bus program, the
mix-bus refusal without FR_STREAM_BUS, a storer that comes later, S_READ_DYN of a ring nobody stores, the option off, a plan with
a fused form and a feedback plan untouched, a plan without a voice), the launch rule's choice for each, and a plain-loop model of
one voice's chain of programs over a sequence of blocks against a dense recurrence: block lengths 64, 1, 37, 63, delays 1, 63, 64
and a signal amount that hits 0, 63, 64 and the bound on a ring at capacity."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "streamtaps_tests.cpp")
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("streamplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp")] + \
       [os.path.join(ROOT, "tests", "cpp", "streamplans.hpp")]
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "streamtaps_tests")


def test_stream_taps_rule_launch_rule_and_chain_model_under_sanitizers():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in [SRC] + DEPS):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        # (the rule's header includes the plan's types, which name HIP's: its headers, no HIP library)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", BIN, SRC], check=True)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
