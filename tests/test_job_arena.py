"""The layout of the batched calls' scratch arenas (spray_amd/csrc/job_arena.h)
on the CPU: tests/cpp/job_arena_test.cpp, built by g++ alone (the header
includes no HIP header) under the address and undefined-behaviour sanitizers
and run as a plain executable."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "job_arena_test.cpp")
GXX = ["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "spray_amd", "csrc")]


def test_layout_program(tmp_path):
    exe = str(tmp_path / "job_arena_test")
    r = subprocess.run([*GXX, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "job_arena_test ok" and not r.stderr


def test_a_take_behind_the_head_has_no_host_side():
    ok = subprocess.run([*GXX, "-fsyntax-only", SRC], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr
    r = subprocess.run([*GXX, "-fsyntax-only", "-DHOST_OF_A_PLAIN_TAKE", SRC],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "host" in r.stderr
