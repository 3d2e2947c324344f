"""The wire ingests' workspace layouts (deneva-plus_amd/csrc/dvcc_wire_layout.h)
checked on the host: tests/cpp/wire_layout_test.cpp, a program of its own
built with the address and undefined-behaviour sanitizers and run as a child
process.  nb around the scan chunk of 3,072 batches and 0, which lays out as 1.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = [0, 1, 2, 3, 3071, 3072, 3073, 6145]


def test_every_field_aligned_disjoint_and_inside_the_reported_size(tmp_path):
    exe = str(tmp_path / "wire_layout_test")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "deneva-plus_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "wire_layout_test.cpp"), "-o", exe])
    r = subprocess.run([exe] + [str(n) for n in NB], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == f"ok {len(NB)}", r.stdout + r.stderr
