"""What a resident launch of block streaming checks before it launches (csrc/kernels.hpp stream_launch_check, the host logic of
kernels.hip launch_bank_stream) as a stand-alone C++ program on the CPU, built with AddressSanitizer and
UndefinedBehaviorSanitizer: tests/cpp/streamcheck_tests.cpp takes a minimal accepted argument set for each of the eight
resident kernels, asserts its workgroup count, breaks every checked field one at a time and asserts the refusal, and compares
the form the check assumes per kernel with the launch rule's record on hand-built plans."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "streamcheck_tests.cpp")
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
DEPS = [os.path.join(CSRC, f) for f in ("streamplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp")]
DEPS.append(os.path.join(ROOT, "tests", "cpp", "streamplans.hpp"))
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "streamcheck_tests")


def test_stream_launch_check_under_sanitizers():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in [SRC] + DEPS):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        # (the check's header names HIP's types: its headers, no HIP library)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", BIN, SRC], check=True)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
