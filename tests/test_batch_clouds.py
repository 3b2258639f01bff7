"""csrc/icp_batch_clouds.h -- the clouds of a batch as the per-cloud kernels number them, their work items, their stretches of the
temporaries, and the packed arguments buffer -- needs no device: tests/batch_clouds_check.cpp runs it as a program of its own under
the address and undefined-behaviour sanitizers (nothing is loaded into this process) against a restatement by brute force."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-point-cloud-registration-with-gpus_amd", "csrc")


def test_batch_clouds_unit_under_sanitizers(tmp_path):
    # the flags the library's host objects are built with, as the Makefile spells them
    flags = subprocess.run(["make", "-s", "--no-print-directory", "-C", CSRC, "--eval", "print-hostflags: ; @echo $(HOSTFLAGS)", "print-hostflags"],
                           capture_output=True, text=True, check=True).stdout.split()
    assert "-O3" in flags and "-D__HIP_PLATFORM_AMD__" in flags, flags
    exe = str(tmp_path / "batch_clouds_check")
    # (the sanitizer flags: see tests/test_wire.py)
    cc = subprocess.run(["g++"] + flags + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-g", "-o", exe,
                                           os.path.join(ROOT, "tests", "batch_clouds_check.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "batch_clouds_check passed" in r.stdout and "FAIL" not in r.stdout
