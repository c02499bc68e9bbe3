"""CPU check of the grid backward's shared scale code (csrc/grid_bwd_scale.h): the stand-alone host
program tests/cpp/grid_bwd_scale_check.cpp emulates the exact pre-pass's and the streaming path's
fp32 summation orders over random multisets of fp16 magnitudes (uniform, banded, sparse, one outlier,
denormals only; chunks of 32 .. 32768 points, and sums placed at the binade edges of `lim`) and asserts
that an accepted streaming sum always gives the exact exponent and that the guard rejects fewer than 1 %
of uniformly random cases. Built once plainly and once with the host sanitizers, each run directly."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO

SRC = os.path.join(REPO, "tests", "cpp", "grid_bwd_scale_check.cpp")


def _cxx():
    for c in ("g++", "clang++", "c++"):
        if shutil.which(c):
            return c
    pytest.fail("no host C++ compiler")


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call([_cxx(), "-std=c++17", *flags, "-o", exe, SRC])
    return exe


def _run(exe, rounds):
    p = subprocess.run([exe, str(rounds)], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    m = re.search(r"cases (\d+) accepted (\d+) rejected (\d+) mismatches (\d+) uniform_cases (\d+) uniform_rejected (\d+)", p.stdout)
    assert m, p.stdout + p.stderr
    return p.returncode, [int(x) for x in m.groups()]


def test_guard_accepts_only_equal_exponents_and_rarely_rejects(tmp_path):
    rc, (cases, accepted, rejected, mismatches, uni, uni_rej) = _run(_build(tmp_path, "scale_check", ["-O2"]), 300)
    assert mismatches == 0
    assert uni >= 2000 and uni_rej * 100 < uni, (uni, uni_rej)  # < 1 % of uniformly random cases
    assert accepted > 0 and rejected > 0 and accepted + rejected == cases  # the edge cases exercise both outcomes
    assert rc == 0


def test_scale_check_clean_under_host_sanitizers(tmp_path):
    exe = _build(tmp_path, "scale_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    rc, (cases, accepted, rejected, mismatches, uni, uni_rej) = _run(exe, 20)
    assert rc == 0 and mismatches == 0
