"""The row bookkeeping of streamed blocks (csrc/streamrows.hpp: fr_stream_block_rows keeps the input store's rules without the
samples) as a stand-alone C++ program on the CPU, built with AddressSanitizer and UndefinedBehaviorSanitizer:
tests/cpp/streamrows_tests.cpp compares it with a model that stores the samples as the reference does -- padding, absent
slots, the vector-count drop, both refusals, and the state staying as it was after a refusal."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "streamrows_tests.cpp")
HDR = os.path.join(ROOT, "libfriendship_amd", "csrc", "streamrows.hpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "streamrows_tests")


def test_stream_rows_bookkeeping_under_sanitizers():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in (SRC, HDR)):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-o", BIN, SRC], check=True)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
