"""cloops_amd/csrc/cl_devbuf.h without a GPU: the header is compiled UNCHANGED with g++ under AddressSanitizer and
UndefinedBehaviorSanitizer into a stand-alone program (tests/c/devbuf_main.cpp) over a counting fake of hipMalloc / hipFree
(tests/c/fake_hip_alloc.cpp), and the program is run as a child process.  It checks the number of live blocks after every step
itself -- ensure / grow, a failing allocation, scope exit, moves, self-move, slices of an arena, a struct of buffers reset by
assignment, a vector of unique_ptr cleared -- so nothing rests on the leak checker.  The sanitizer runtimes are linked statically:
the program needs nothing preloaded and does not mind what is."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_devbuf_under_asan_and_ubsan(tmp_path):
    if not os.path.exists(os.path.join(ROCM_INC, "hip", "hip_runtime_api.h")):
        pytest.skip("no ROCm headers here")
    exe = str(tmp_path / "devbuf_main")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__",
                           "-I" + ROCM_INC, "-I" + os.path.join(ROOT, "cloops_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "devbuf_main.cpp"), os.path.join(ROOT, "tests", "c", "fake_hip_alloc.cpp"),
                           "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert run.returncode == 0 and run.stdout.decode().strip() == "devbuf ok", run.stderr.decode()[-2000:]

