"""The batch builder's size guard behind the compiled kernels' 32-bit column addressing (kyv_wave.h gcol adds a
column's offset and the row in 32 bits): the decision itself, at entry counts around 2^32, with the count supplied
(a batch of that size is 32 GiB of column entries)."""
from kyverno_amd import _lib as K

LIMIT = 0xFFFFFFF0  # kyv_layout.h COL_ENTRIES_MAX: 2^32 less NONE, the table's sentinel entry and a margin


def test_guard_accepts_below_and_refuses_at_2_pow_32():
    fit = K.lib().kyv_col_entries_fit32
    assert fit(0) == 1
    assert fit(1) == 1
    assert fit(LIMIT) == 1            # the largest table a batch may hold
    assert fit(LIMIT + 1) == 0
    assert fit(2**32 - 1) == 0        # just below 2^32: offset + row + sentinel would not fit
    assert fit(2**32) == 0
    assert fit(2**32 + 5) == 0        # a count whose low 32 bits are small must not pass
    assert fit(2**40) == 0


def test_every_accepted_offset_plus_row_fits_32_bits():
    """offset + row of any entry of an accepted table, the sentinel included, is below 2^32 and is not NONE"""
    assert K.lib().kyv_col_entries_fit32(LIMIT) == 1
    last = LIMIT  # index of the sentinel entry (colv holds entries + 1)
    assert last < 2**32 - 1
