"""FR_STREAM_HISTORY on the host (csrc/streamplan.hpp, csrc/kernels.hpp) as a stand-alone C++ program on the CPU, built with
AddressSanitizer and UndefinedBehaviorSanitizer: tests/cpp/streamhist_tests.cpp checks the serving rule on hand-built plans (a
delayed read of an input row in a voice's, a bus and a loop program, its slot, a signal amount with and without FR_STREAM_DYN
and a proven bound, the look-back's limit, the option off), the launch rule (hist on top of the cascade, the history's capacity),
stream_launch_check of the hist form with every checked field broken one at a time (the value after dyn stays unnamed and
refused), and a plain-loop model of the history at capacity against a model that keeps every sample."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "streamhist_tests.cpp")
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("streamplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp")] + \
       [os.path.join(ROOT, "tests", "cpp", "streamplans.hpp")]
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "streamhist_tests")


def test_stream_hist_rule_launch_check_and_history_under_sanitizers():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in [SRC] + DEPS):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        # (the rule's header includes the plan's types, which name HIP's: its headers, no HIP library)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", BIN, SRC], check=True)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
