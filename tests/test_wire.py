"""csrc/icp_wire.cpp -- mailbox lines, row formats, the row sweep, the adders, the tag allocator -- needs no device: tests/wire_check.cpp
runs it as a program of its own under the address and undefined-behaviour sanitizers (nothing is loaded into this process)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fast-point-cloud-registration-with-gpus_amd", "csrc")


def test_wire_unit_under_sanitizers(tmp_path):
    # the flags the library's host objects are built with, as the Makefile spells them
    flags = subprocess.run(["make", "-s", "--no-print-directory", "-C", CSRC, "--eval", "print-hostflags: ; @echo $(HOSTFLAGS)", "print-hostflags"],
                           capture_output=True, text=True, check=True).stdout.split()
    assert "-O3" in flags and "-D__HIP_PLATFORM_AMD__" in flags, flags
    exe = str(tmp_path / "wire_check")
    # -fno-sanitize-recover: a finding of the undefined-behaviour sanitizer ends the program with an error instead of a message.
    # -static-lib*san: ASan refuses to start when its shared runtime is not the first library in the process (its link-order
    # check), which any preloaded library breaks; linked into the program there is no such order to check.
    cc = subprocess.run(["g++"] + flags + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-g", "-o", exe,
                                           os.path.join(ROOT, "tests", "wire_check.cpp"), os.path.join(CSRC, "icp_wire.cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wire_check passed" in r.stdout and "FAIL" not in r.stdout
