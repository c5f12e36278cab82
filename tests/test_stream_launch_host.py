"""The launch rule of block streaming on the host (csrc/streamplan.hpp stream_path, stream_launch, plain_stream_launch) as a
stand-alone C++ program on the CPU, built with AddressSanitizer and UndefinedBehaviorSanitizer: tests/cpp/streamlaunch_tests.cpp
checks each of the seven resident kernels on a hand-built plan that calls for it (doorbell form, rows, tables, limits,
workgroups), the precedence between them, the loop limits against a direct count, the plain path exactly where fr_stream_begin
has always taken it, and the one-bank chunk dealing against the loop fr_stream_begin used to have."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "streamlaunch_tests.cpp")
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("streamplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp")]
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "streamlaunch_tests")


def test_stream_launch_rule_under_sanitizers():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in [SRC] + DEPS):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        # (the rule's header includes the plan's types, which name HIP's: its headers, no HIP library)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", BIN, SRC], check=True)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
