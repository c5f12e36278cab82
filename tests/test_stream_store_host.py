"""FR_STREAM_STORE on the host (csrc/streamstore.hpp) as a stand-alone C++ program on the CPU, built with AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/streamstore_tests.cpp checks the slots a stream that stores its rows streams and their
limit, append or relaunch at every boundary of make_room's three branches (bounded and unbounded; store_room against make_room
written out again over 20 000 random states), the floor, streamrows.hpp's books opened from a store state and then 200 random
sequences of calls, blocks, seeks and re-openings whose books and streamed values must equal a store that keeps the samples, and
the inert reasons.  tests/cpp/bringup_tests.cpp pins the call of zero own frames (csrc/callplan.hpp bring_up_form with call_windows)
over hand-built plans: the look-back window, and each case in which nothing is launched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "streamstore_tests.cpp")
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("streamstore.hpp", "streamrows.hpp", "streamplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp")]
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "streamstore_tests")
BRINGUP_SRC = os.path.join(ROOT, "tests", "cpp", "bringup_tests.cpp")
BRINGUP_BIN = os.path.join(ROOT, "tests", "cpp", "_build", "bringup_tests")


def _run(src, deps, binary):
    if not os.path.exists(binary) or os.path.getmtime(binary) < max(os.path.getmtime(p) for p in [src] + deps):
        os.makedirs(os.path.dirname(binary), exist_ok=True)
        # (the rule's header includes the plan's types, which name HIP's: its headers, no HIP library)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", binary, src], check=True)
    p = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]


def test_stream_store_rule_under_sanitizers():
    _run(SRC, DEPS, BIN)


def test_the_call_of_zero_own_frames_under_sanitizers():
    _run(BRINGUP_SRC, [os.path.join(CSRC, f) for f in ("callplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp")], BRINGUP_BIN)
