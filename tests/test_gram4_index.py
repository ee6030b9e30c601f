"""The pair-shared M-word address of gram4's main path (gram4_index.hpp, K = 3) on the CPU: tests/native/gram4_index_check.cpp walks every
class count 2..30, four places of M in LDS and every class tuple through g4i_even / g4i_odd against the three-term address, and checks that
every operand of a 24-bit multiply-add is below 2^24."""
import os
import subprocess

from conftest import ROOT


def test_pair_index_equals_three_term_address(tmp_path):
    exe = str(tmp_path / "gram4_index_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "gram4_index_check.cpp")])
    out = subprocess.check_output([exe]).decode()
    assert out.startswith("OK"), out
    # four offsets x sum of C^4 over C = 2..30
    assert int(out.split("tuples=")[1]) == 4 * sum(c ** 4 for c in range(2, 31)), out
