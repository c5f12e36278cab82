"""FR_STREAM_GENERAL on the host (csrc/streamplan.hpp) as a stand-alone C++ program on the CPU, built with AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/streamgeneral_tests.cpp checks the schedule validation on well-formed schedules and on each
malformed kind, the one-item schedules of balanced 32- and 64-partial banks, the chunk dealing with schedule banks mixed in, the
serving rule on hand-built banks, and a plain-loop model of the kernel's schedule renderer (16 waves, the ladder, the stack)
against a direct evaluation of the tree the schedule describes, bit for bit, for every item size and both operand orders."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "streamgeneral_tests.cpp")
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("streamplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp")]
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "streamgeneral_tests")


def test_stream_general_schedules_rule_and_model_under_sanitizers():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in [SRC] + DEPS):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        # (the rule's header includes the plan's types, which name HIP's: its headers, no HIP library)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", BIN, SRC], check=True)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
