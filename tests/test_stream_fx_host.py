"""FR_STREAM_EFFECTS on the host (csrc/streamplan.hpp, csrc/kernels.hpp) as a stand-alone C++ program on the CPU, built with
AddressSanitizer and UndefinedBehaviorSanitizer: tests/cpp/streamfx_tests.cpp checks the serving rule on hand-built plans without
a bank launch (groups and segments, the wrap over four workgroups, taps and row copies that follow their loop, bus detection,
every refusal with its text, the option off), the launch rule (fx exactly for a plan without a voice, its workgroups, a history
of at least a block), the kernels' numbers, names and forms (the values after dyn, hist and fx refused; the nine older forms
unchanged), stream_launch_check of the fx form with every checked field broken one at a time, and a plain-loop model of one
segment's block against a dense recurrence for comb_5, one_pole and tap_behind."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "streamfx_tests.cpp")
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("streamplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp")] + \
       [os.path.join(ROOT, "tests", "cpp", "streamplans.hpp")]
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "streamfx_tests")


def test_stream_fx_rule_launch_check_and_segment_model_under_sanitizers():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in [SRC] + DEPS):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        # (the rule's header includes the plan's types, which name HIP's: its headers, no HIP library)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", BIN, SRC], check=True)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
