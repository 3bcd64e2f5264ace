"""A host RESTATEMENT of the dense walk of the one-tile update kernel (csrc/ge_train.hip: next_live_slot,
add_live_rows, add_live_item): the lowest set bit of the liveness mask is taken and cleared, W times a group, a group
of 4 when at most 4 live slots are left and of RW otherwise.  It shares no code with the kernel: it pins the algorithm
down for every 16-bit mask -- exactly the live slots, in ascending order, in as few groups as the widths allow.  That
the kernel does this on the device is checked by the partly-live cases of tests/test_gpu_update_onetile.py."""
import pytest

ITEM_CAP = 16


def next_live_slot(mask):
    b = (mask & -mask).bit_length() - 1        # s_ff1
    return b, mask & (mask - 1)


def walk(mask, rw):
    """-> the groups of slots add_live_item<rw> requests for `mask`, in order"""
    rs = min(rw, 4)
    groups = []
    while mask:
        w = rw if (rw > rs and bin(mask).count("1") > rs) else rs
        g = []
        for _ in range(w):
            if mask:
                b, mask = next_live_slot(mask)
                g.append(b)
        groups.append(g)
    return groups


@pytest.mark.parametrize("rw", [2, 4, 8, 16])
def test_dense_walk_visits_exactly_the_live_slots_in_ascending_order(rw):
    for mask in range(1 << ITEM_CAP):
        groups = walk(mask, rw)
        seen = [b for g in groups for b in g]
        live = [b for b in range(ITEM_CAP) if (mask >> b) & 1]
        assert seen == live, (mask, rw)
        n = len(live)
        # every group but the last is full; up to 4 live slots take one group of 4, more take ceil(n / rw) groups of rw
        # and, when at most 4 are left over, a group of 4 for those
        assert all(len(g) > 0 for g in groups)
        if n <= min(rw, 4):
            assert len(groups) == (1 if n else 0)
        else:
            assert len(groups) == -(-n // rw), (mask, rw)


def test_sixteen_listed_seven_live_is_one_group_at_eight():
    assert walk(0b1010_0101_0011_0100, 8) == [[2, 4, 5, 8, 10, 13, 15]]
