"""The region arithmetic of gram4's claims (gram4_claims.hpp) on the CPU: tests/native/gram4_claims_check.cpp walks every claim index of a grid of
(haystack length, large and small region size, split point) and checks that the regions tile the haystack exactly once, in ascending order,
each at a multiple of its own size and none across a multiple of 2 GiB."""
import os
import subprocess

from conftest import ROOT


def test_claims_tile_the_haystack_once_in_order(tmp_path):
    exe = str(tmp_path / "gram4_claims_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "gram4_claims_check.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("OK"), out
    assert int(out.split("plans=")[1].split()[0]) > 1000 and int(out.split("regions=")[1]) > 1000000, out
