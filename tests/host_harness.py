"""Building and running the host programs of tests/san/ (and the fuzzers) under a sanitizer: the one compiler line, the one way to
run a program and read its lines, and the status codes of include/lewton_amd.h (tests/test_host_kernel_harness.py holds them
against the header)."""
import os
import subprocess

from common import ROOT

CS = os.path.join(ROOT, "lewton_amd", "csrc")
SAN = os.path.join(ROOT, "tests", "san")
HIP_INC = "/opt/rocm/include"
OK, NULL_ARG, DEVICE, CAPACITY, STATE_MISMATCH, UNSUPPORTED = 0, 32, 33, 34, 35, 36


def compile_to(exe, sources, sanitize="address,undefined", extra=()):
    """compiles `sources` into the program `exe` and returns it; `extra`: a program's own flags"""
    assert os.path.isdir(os.path.join(HIP_INC, "hip")), "the CPU suite compiles the host side against the HIP headers"
    recover = [] if sanitize == "thread" else ["-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=" + sanitize] + recover +
                          ["-ffp-contract=off", "-DLW_CHECK_NARROW", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC] + list(extra) + list(sources) +
                          ["-lpthread", "-o", exe])
    return exe


def build(tmp_path_factory, name, sources, sanitize="address,undefined", extra=()):
    """compile_to, into the program `name` in a temporary directory of its own"""
    return compile_to(str(tmp_path_factory.mktemp(name) / name), sources, sanitize, extra)


def run(exe, *args, timeout=600, ok=True, env=None):
    """the lines `exe` prints; ok=False: whatever its exit status, for a test that looks at a refusal's lines itself"""
    r = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], capture_output=True, text=True, timeout=timeout, env=env)
    if ok:
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout.splitlines()
