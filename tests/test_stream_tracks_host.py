"""FR_STREAM_TRACKS on the host (csrc/leafprog.hpp, csrc/streamplan.hpp, csrc/kernels.hpp) as a stand-alone C++ program on the CPU,
built with AddressSanitizer and UndefinedBehaviorSanitizer: tests/cpp/streamtracks_tests.cpp checks the leaf-program compiler with
track operands on the leaf BankMatcher makes of synth.track_tree's partial and on hand-built shapes, a plain-loop model of the
interpreter's walk with the one-partial-ahead loads and the double buffer they are parked in against a direct evaluation of the
shape over the dense matrix under the slot limit, bit for bit, and the serving rule, the launch rule and the launch check of the
two track kernels (the program links graph.cpp, match.cpp, stage.cpp and leafjit.cpp; the simulator has no run-time compiler)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "streamtracks_tests.cpp")
CSRC = os.path.join(ROOT, "libfriendship_amd", "csrc")
LINKED = [os.path.join(CSRC, f) for f in ("graph.cpp", "match.cpp", "stage.cpp", "leafjit.cpp")]
DEPS = LINKED + [os.path.join(CSRC, f) for f in ("leafprog.hpp", "leafshape.hpp", "streamplan.hpp", "stage.hpp", "graph.hpp", "match.hpp", "range.hpp", "kernels.hpp",
                                                 "jit.hpp")] + [os.path.join(ROOT, "tests", "cpp", "streamplans.hpp")]
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "streamtracks_tests")


def test_track_operands_model_rule_and_check_under_sanitizers():
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(p) for p in [SRC] + DEPS):
        os.makedirs(os.path.dirname(BIN), exist_ok=True)
        # (-ffp-contract=off: the model's arithmetic rounds every operation, as the kernels' does)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-pthread", "-o", BIN, SRC] + LINKED + ["-ldl"], check=True)
    p = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and " passed; 0 failed" in p.stdout, p.stdout[-4000:] + p.stderr[-4000:]
