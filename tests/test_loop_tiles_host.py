"""The rule that decides whether a feedback plan's strided launches render tiles staged in LDS (csrc/callplan.hpp loop_tile,
FR_LOOP_TILES) as a stand-alone C++ program on the CPU, built with AddressSanitizer and UndefinedBehaviorSanitizer:
tests/cpp/looptile_tests.cpp checks the frames per tile of every stride 1..64, stride 65, each refusal with its reason on
hand-built plans, the option off and a plan without feedback."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "looptile_tests.cpp")
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("callplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp")]
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "looptile_tests")


def test_loop_tile_rule_under_sanitizers():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in [SRC] + DEPS):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        # (the rule's header includes the plan's types, which name HIP's: its headers, no HIP library)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", BIN, SRC], check=True)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
