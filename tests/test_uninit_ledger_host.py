"""The ledger of tests/test_gpu_uninitialised.py, without a GPU: every function include/daachorse_amd.h declares is either host-only
(uninit_cases.HOST_ONLY: it hands out no device scratch, staging or result buffer) or driven by at least one case of
uninit_cases.CASES.  An entry point added to the header fails this test until somebody registers it.  And the option the cases run
under: its range, its default and the per-handle refusal."""
import os
import re

import pytest

import daachorse_amd as da

import uninit_cases as uc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "daachorse_amd.h")


def declared(text):
    """the names of the functions a header declares: `daac_<name>(` at the start of a declaration's line, comments taken out"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return set(re.findall(r"^[A-Za-z_][\w \t\*]*?\b(daac_\w+)\s*\(", text, flags=re.M))


def test_the_parser_reads_declarations():
    sample = "/* daac_not_me(int) */\nuint32_t daac_abi_version(void);\nconst daac_match *daac_matches_data(const daac_matches *m);\n" \
             "daac_status daac_scan(daac_pma *pma,\n                      int mode);\ntypedef struct daac_pma daac_pma;\n"
    assert declared(sample) == {"daac_abi_version", "daac_matches_data", "daac_scan"}


def _names():
    with open(HEADER) as f:
        return declared(f.read())


def unregistered(names, cases):
    """the declared names that are neither host-only nor driven by one of `cases`"""
    driven = {e for c in cases.values() for e in c.entries}
    assert not (uc.HOST_ONLY & driven), sorted(uc.HOST_ONLY & driven)
    assert not (uc.HOST_ONLY - names) and not (driven - names), ("names the header does not declare", sorted((uc.HOST_ONLY | driven) - names))
    return names - uc.HOST_ONLY - driven


def test_every_entry_point_is_host_only_or_driven_by_a_case():
    names = _names()
    assert len(names) >= 70 and {"daac_scan", "daac_tokens_decode", "daac_stream_feed_compact", "daac_set_option"} <= names, sorted(names)
    missing = unregistered(names, uc.CASES)
    assert not missing, f"entry points that no case of tests/uninit_cases.py drives and HOST_ONLY does not list: {sorted(missing)}"


def test_the_ledger_fails_when_a_case_is_removed():
    """the same check over the table without the one case behind daac_scan_count_multi, and over a header with one function more"""
    only = [n for n, c in uc.CASES.items() if "daac_scan_count_multi" in c.entries]
    assert len(only) == 1
    assert unregistered(_names(), {n: c for n, c in uc.CASES.items() if n not in only}) == {"daac_scan_count_multi"}
    assert unregistered(_names() | {"daac_new_call"}, uc.CASES) == {"daac_new_call"}


def test_every_case_names_what_it_drives():
    assert len(uc.CASES) > 150
    for name, c in uc.CASES.items():
        assert c.entries and callable(c.run) and callable(c.want), name


def test_debug_fill_range_default_and_per_handle_refusal():
    try:
        for ok in (0, 1, 0xA5, 255, -1):
            da.set_option("debug_fill", ok)
        for bad in (-2, 256, 1 << 40, -(1 << 40)):
            with pytest.raises(da.DaachorseError) as ei:
                da.set_option("debug_fill", bad)
            assert ei.value.code == 1 and "debug_fill" in str(ei.value), bad
        p = da.DoubleArrayAhoCorasick.new([b"ab", b"b"])
        for value in (0, 0xA5, -1, None):   # (None: taking an override away is refused as well, as for pool)
            with pytest.raises(da.DaachorseError) as ei:
                p.set_option("debug_fill", value)
            assert ei.value.code == 1 and "allocator" in str(ei.value), value
    finally:
        da.set_option("debug_fill", -1)
