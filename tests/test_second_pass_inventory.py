"""No GPU: the launch inventory of tests/second_pass.py matches the sources, names tests that exist, and its helpers hold their promises."""
import os
import re

import numpy as np
import pytest

from tests import second_pass as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_capped_launch_site_is_registered():
    """a new `cu_count()` launch or `group_grid` call fails here until it is entered in second_pass.INVENTORY with the test that takes
    it past its cap"""
    assert SP.counted_sites() == SP.inventory_counts()


def test_inventory_names_tests_that_exist_and_size_from_the_device():
    for s in SP.INVENTORY:
        if s.test is None:
            assert s.exempt and s.note, s  # only an exempt site goes without a test, and its entry says why
            continue
        assert not s.exempt, s
        path, name = s.test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        m = re.search(rf"^def {re.escape(name)}\(.*?(?=^def |^@pytest|\Z)", text, re.S | re.M)
        assert m, s.test
        if path == SP.NEW:  # the new tests size their columns from the device's CU count and say so
            assert "device_info()" in text and re.search(r"assert n\w* > ", m.group(0)), s.test


def test_every_fixed_grid_site_is_registered_with_a_test_that_exists():
    """a new `X_LIST_BLOCKS` / `X_BIG_BLOCKS` grid fails here until it is entered in second_pass.FIXED_GRID_SITES with the test that
    lists more units than the grid has work-groups; the named test exists and sizes its list from the constant"""
    assert SP.counted_fixed_sites() == SP.fixed_inventory() and len(SP.FIXED_GRID_SITES) == 5
    for s in SP.FIXED_GRID_SITES:
        assert SP.fixed_grid(s.constant) == 1024, s
        path, name = s.test.split("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        m = re.search(rf"^def {re.escape(name)}\(.*?(?=^def |^@pytest|\Z)", text, re.S | re.M)
        assert m and re.search(r"BLOCKS", m.group(0)) and re.search(r"rotating_tiling|shuffled_tiling", m.group(0)), s.test


def test_second_trip_rows():
    assert SP.second_trip_rows(256, 32, 64) == 256 * 32 * 64 * 5 // 4 + 37 and SP.second_trip_rows(8, 8, 1, extra=5) == 69
    with pytest.raises(AssertionError):
        SP.second_trip_rows(256, 32, 16, extra=32)


def test_tilings_never_bring_the_same_row_back():
    order = SP.shuffled_tiling(96, 5000, seed=1, groups=960)  # (a stride that is a multiple of the base: arange % 96 would repeat)
    assert order.min() == 0 and order.max() == 95 and len(np.unique(order[:96])) == 96
    assert np.array_equal(order, SP.shuffled_tiling(96, 5000, seed=1, groups=960))
    assert np.array_equal(order[SP.first_rows(order, 96)], np.arange(96))
    with pytest.raises(AssertionError):
        SP.shuffled_tiling(4, 5000, seed=1, groups=960)  # four base rows: a quarter of the second units would equal the first
    for n_base in (2, 3, 4, 7):
        for groups in (8, 9, 11, 12, 1024):
            o = SP.rotating_tiling(n_base, 3 * groups + 5, groups)
            assert (o[:-groups] != o[groups:]).all() and set(o.tolist()) == set(range(n_base))


def test_same_bits():
    assert SP.same_bits(np.array([0.0, np.nan]), np.array([0.0, np.nan])) and not SP.same_bits(np.array([0.0]), np.array([-0.0]))
