"""FR_STREAM_DYN on the host (csrc/streamplan.hpp) as a stand-alone C++ program on the CPU, built with AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/streamdyn_tests.cpp checks the serving rule on hand-built plans (a signal delay of one
voice's ring and of two voices' with and without FR_STREAM_BUS, of a ring a program stores, inside a loop program, of an input
row, with an observed bound; the look-back), the launch rule (dyn on top of the cascade, the schedule table only with schedule
banks, unchanged launches for plans without a signal delay), and a plain-loop model of the interpreter's two ops on a ring at
capacity against the Delay's definition over the whole history, for hostile amounts, in both semantics."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "streamdyn_tests.cpp")
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("streamplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp")]
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "streamdyn_tests")


def test_stream_dyn_rule_launch_and_ops_under_sanitizers():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in [SRC] + DEPS):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        # (the rule's header includes the plan's types, which name HIP's: its headers, no HIP library)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", BIN, SRC], check=True)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
