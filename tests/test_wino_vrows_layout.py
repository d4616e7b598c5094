"""The shared-row V layout of the row-direct tower (wino.h wino_vr_*, AZ_WINO_VROWS) from the address
tables that az_wino_vrows_layout tabulates out of the kernel's own formulas: coverage of the transform's
writes under both item schedules, the B-fragment reads against the entry formula, and LDS bank conflicts
with gfx950's lane groups.  No GPU."""
import numpy as np
import pytest

import azchess.agent as AG

ROWS, OCT, TC, PTS = 10, 4, 4, 4
# gfx950 LDS service groups: a ds_read_b128 in four groups over 64 banks, a 32-bit access in two over 32
G128 = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
        [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
G128 = G128 + [[l + 32 for l in g] for g in G128]
G32 = [list(range(32)), list(range(32, 64))]


@pytest.fixture(scope="module")
def lay():
    return AG.wino_vrows_layout()


def entry(b, r, o, tc):
    """byte offset of entry (column point, padded row, channel octet, tile column) within a plane"""
    return ((2 * b + (r & 1)) * 5 + (r >> 1)) * 256 + (4 * (o ^ (2 * ((r >> 1) & 1))) + tc) * 16


def plane_entry(pl, plane, b, r, o, tc):
    """the entry in the hi (0) or lo (1) plane: the lo plane holds it at tile column tc ^ 2"""
    return pl * plane + entry(b, r, o, tc ^ (2 * pl))


def ways(addrs, width, banks):
    """the worst number of distinct dwords of one bank among the given lanes' accesses (`width` bytes each);
    lanes at the same address share one access"""
    per = {}
    for a in addrs:
        for k in range(width // 4):
            d = int(a) // 4 + k
            per.setdefault(d % banks, set()).add(d)
    return max(len(v) for v in per.values())


def test_dims_and_entries(lay):
    plane, buf, r16, cb = (int(x) for x in lay["dims"])
    assert (plane, buf, r16, cb) == (10240, 20480, (256 // 4 + 2) * 16, 4)
    all_e = sorted(entry(b, r, o, tc) for b in range(PTS) for r in range(ROWS) for o in range(OCT) for tc in range(TC))
    assert all_e == list(range(0, plane, 16))                 # 640 entries tile a plane exactly


@pytest.mark.parametrize("sched", [0, 1])
def test_every_entry_written_once(lay, sched):
    """per chunk every (b, r in 1..8, octet, tc, channel pair, plane) word is written by exactly one (wave,
    item, lane); rows 0 and 9 by none"""
    plane = int(lay["dims"][0])
    items = lay["item"][sched]
    used = [int(q) for q in items.ravel() if q >= 0]
    assert sorted(used) == list(range(16))                   # the waves' items are the 16 wave-items, once each
    nw = 8 if sched else 4
    assert (items[nw:] == -1).all() and (items[:nw, :16 // nw] >= 0).all() and (items[:nw, 16 // nw:] == -1).all()
    count = np.zeros(2 * plane // 4, np.int32)
    owner = {}
    for w in range(8):
        for it in range(4):
            q = int(items[w, it])
            if q < 0:
                continue
            for lane in range(64):
                r, ch, tc = 1 + (q >> 1), 16 * (q & 1) + (lane & 15), lane >> 4
                for b in range(PTS):
                    a = int(lay["write"][q, lane, b])
                    want = plane_entry(lane & 1, plane, b, r, ch >> 3, tc) + ((ch & 7) >> 1) * 4
                    assert a == want, (q, lane, b, a, want)
                    count[a // 4] += 1
                    owner[a] = (w, it, lane)
    want = np.zeros_like(count)
    for pl in range(2):
        for b in range(PTS):
            for r in range(ROWS):
                for o in range(OCT):
                    for tc in range(TC):
                        base = plane_entry(pl, plane, b, r, o, tc) // 4
                        want[base:base + 4] = 1 if 1 <= r <= 8 else 0
    assert np.array_equal(count, want)
    assert len(owner) == int(want.sum())


def test_reads_are_the_entries(lay):
    for i in range(4):
        for b in range(PTS):
            for lane in range(64):
                h, tr, tc = lane >> 4, (lane & 15) >> 2, lane & 3
                for pl in range(2):
                    assert int(lay["read"][pl, i, b, lane]) == plane_entry(pl, int(lay["dims"][0]), b, 2 * tr + i, h, tc)


def test_bank_conflicts(lay):
    """B-fragment reads and V writes one-way; the items' ACT reads at most two-way"""
    for i in range(4):
        for b in range(PTS):
            for g in G128:
                assert ways(lay["read"][0, i, b, g], 16, 64) == 1 and ways(lay["read"][1, i, b, g], 16, 64) == 1, (i, b)
    for q in range(16):
        for k in range(4):
            for g in G32:
                assert ways(lay["write"][q, g, k], 4, 32) == 1, (q, k)
                assert ways(lay["act"][q, g, k], 4, 32) <= 2, (q, k)


def test_act_reads_are_the_patch_columns(lay):
    """the item's four reads: columns 2 tc - 1 .. 2 tc + 2 of board row r - 1, an off-board column clamped to
    an on-board one (multiplied by 0 in the transform), the lane's channel"""
    r16, cb = int(lay["dims"][2]), int(lay["dims"][3])
    for q in range(16):
        for lane in range(64):
            y, ch, tc = q >> 1, 16 * (q & 1) + (lane & 15), lane >> 4
            for j in range(4):
                x = 2 * tc - 1 + j
                a = int(lay["act"][q, lane, j])
                sq, rem = divmod(a, r16)
                assert rem == ch * cb and sq // 8 == y
                if 0 <= x < 8:
                    assert sq % 8 == x
                else:
                    assert (tc, j) in ((0, 0), (3, 3)) and 0 <= sq % 8 < 8
