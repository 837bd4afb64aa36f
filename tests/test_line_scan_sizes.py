"""CPU test (no GPU): the work areas of the three users of csrc/line_scan.inc keep their sizes -- a header, one element per line (+ 1),
one block total per 1024 lines and at least one.  The literals are what the library returned before the scans were made one template."""
import pytest

SIZES = {
    # nlines: (fibd_str_work_size, fibd_str_select_work_size, fibd_prob_work_size)
    0: (32, 64, 56),
    1: (40, 88, 56),
    1024: (8224, 24640, 24608),
    1025: (8240, 24688, 24648),
    525315: (4206656, 12619936, 12615800),
}


@pytest.mark.parametrize("nlines", sorted(SIZES))
def test_work_sizes_are_what_they_were(fj, nlines):
    assert (fj.str_work_size(nlines), fj.str_select_work_size(nlines), fj.prob_work_size(nlines)) == SIZES[nlines]
