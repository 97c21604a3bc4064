"""ffd_host_cu_masks: the CU masks of the stream partitions (host only, no device needed)."""
import ctypes as C

import pytest

from fastfourierdiffusion_amd import _native as N

SPREAD, XCD = 0, 1


def masks(n_cus, n_xcds, layout, parts):
    words = (n_cus + 31) // 32
    buf = (C.c_uint32 * (parts * words))()
    rc = N.lib().ffd_host_cu_masks(n_cus, n_xcds, layout, parts, buf)
    return rc, [{b for b in range(32 * words) if buf[p * words + b // 32] >> (b % 32) & 1} for p in range(parts)]


@pytest.mark.parametrize("parts", [2, 4])
@pytest.mark.parametrize("layout", [SPREAD, XCD], ids=["spread", "xcd"])
def test_masks_are_disjoint_complete_and_even(layout, parts):
    n_cus, n_xcds = 256, 8
    rc, got = masks(n_cus, n_xcds, layout, parts)
    assert rc == 0
    assert set().union(*got) == set(range(n_cus))            # complete, and nothing past the chip
    assert sum(len(g) for g in got) == n_cus                 # disjoint
    assert all(len(g) == n_cus // parts for g in got)        # even
    for g in got:                                            # mask bit b: CU b // n_xcds of XCD b % n_xcds
        per_xcd = [sum(1 for b in g if b % n_xcds == x) for x in range(n_xcds)]
        if layout == SPREAD:  # the same number of CUs of every XCD
            assert per_xcd == [n_cus // n_xcds // parts] * n_xcds
        else:                 # whole XCDs
            assert sorted(per_xcd) == [0] * (n_xcds - n_xcds // parts) + [n_cus // n_xcds] * (n_xcds // parts)


def test_spread_halves_are_the_two_halves_of_the_mask():
    """The layout the sampling loops use, as measured on the chip (tools/partition_probe.py): words 0-3 and 4-7."""
    rc, (a, b) = masks(256, 8, SPREAD, 2)
    assert rc == 0 and a == set(range(128)) and b == set(range(128, 256))


@pytest.mark.parametrize("args", [
    (256, 8, SPREAD, 3),    # 32 CUs per XCD do not divide by 3
    (256, 8, XCD, 3),       # nor do 8 XCDs
    (304, 8, SPREAD, 4),    # 38 CUs per XCD do not divide by 4
    (250, 8, SPREAD, 2),    # the CUs do not divide over the XCDs
    (256, 8, 2, 2),         # unknown layout
    (0, 8, SPREAD, 2), (256, 0, SPREAD, 2), (256, 8, SPREAD, 0),
], ids=str)
def test_counts_that_do_not_divide_are_rejected(args):
    buf = (C.c_uint32 * 64)()
    assert N.lib().ffd_host_cu_masks(*args, buf) == -1


def test_null_output_is_rejected():
    assert N.lib().ffd_host_cu_masks(256, 8, SPREAD, 2, None) == -1


def test_other_chip_sizes():
    rc, got = masks(304, 8, SPREAD, 2)  # 38 CUs per XCD: 19 each
    assert rc == 0 and [len(g) for g in got] == [152, 152] and not (got[0] & got[1])
    rc, got = masks(64, 8, XCD, 8)
    assert rc == 0 and all(len(g) == 8 and len({b % 8 for b in g}) == 1 for g in got)


def test_knob_and_status_getter_exist():
    lib = N.lib()
    v = C.c_int(-1)
    assert lib.ffd_tune_get(b"partitions", C.byref(v)) == 0 and v.value in (0, 1)
    for ok in (0, 1, 2):
        assert lib.ffd_tune(b"partitions", ok) == 0
    assert lib.ffd_tune(b"partitions", 3) == -1 and lib.ffd_tune(b"partitions", -1) == -1
    assert lib.ffd_tune(b"reset", 0) == 0
    assert lib.ffd_partition_status(None, C.byref(v)) == -1


def test_plan_query_exists_and_refuses_a_null_context():
    """ffd_partition_plan without a context is FFD_ERR_INVALID whatever the other arguments, and leaves *info alone (the
    argument errors that need a context -- info NULL, B < 1, an entry that names no loop -- are asserted on the device, in
    tests/test_partition_plans_gpu.py)."""
    lib = N.lib()
    info = N.PartitionInfo()
    info.parts = 77
    for B, entry in ((2, N.FFD_SOLVER_EULER_MARUYAMA), (0, N.FFD_SOLVER_ODE_EULER), (2, 99)):
        assert lib.ffd_partition_plan(None, B, entry, C.byref(info)) == -1
    assert lib.ffd_partition_plan(None, 2, N.FFD_SOLVER_EULER_MARUYAMA, None) == -1
    assert info.parts == 77
    # the layout include/ffd.h declares: eleven ints, the long long on its 8-byte boundary, the two names
    assert C.sizeof(N.PartitionHalf) == 168 and N.PartitionHalf.part_floats.offset == 48 and N.PartitionHalf.ffn.offset == 56
    assert C.sizeof(N.PartitionInfo) == 16 + 3 * 168 and N.PartitionInfo.whole.offset == 16 + 2 * 168
