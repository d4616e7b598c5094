"""The two-board tower's layout (wino.h wino_b2_*, tower.hip tower32w_boards2, AZ_WINO_BOARDS=2) from the
tables that az_wino_boards_layout and az_wino_vrows_layout tabulate out of the kernel's own constants and
address functions: the in-step item schedule, the items' reads and the epilogue's accesses of the global
activations, and the LDS regions.  The kernel keeps no activation slice in LDS (the items read the global
buffers directly), so what is checked of a chunk's 32-channel slice is that the items' global reads cover
it; the slice-coverage and bank-conflict checks belong here once a slice is staged in LDS.  The LDS regions
come from the constants the kernel is compiled with (tower.hip WINO_B2_*); that the ACT overlay lies inside V
is also a static_assert there, which is the guard that cannot go stale.  No GPU."""
import numpy as np
import pytest

import azchess.agent as AG

LDS_MAX = 163840


@pytest.fixture(scope="module")
def lay():
    return AG.wino_boards_layout(), AG.wino_vrows_layout()


def test_dims(lay):
    b2, vr = lay
    act, wg, vbuf, ov_off, ov_bytes, aux_off, aux_bytes, lds = (int(x) for x in b2["dims"])
    r16 = int(vr["dims"][2])
    assert act == 64 * r16 == 67584 and wg == 4 * act == 270336 and vbuf == int(vr["dims"][1]) == 20480
    assert lds <= LDS_MAX
    print("two-board tower LDS: %d B" % lds)


def test_items_cover_both_boards_once(lay):
    """per chunk the waves' items are the 16 wave-items of either board, once each; a wave's items come first
    in its row and fit the steps (item k is read at step k and written at step k + 1 <= 11); waves 0-3 take
    the same number each, at least their share, and so do waves 4-7.  With the shared-row tables that is
    every (square, channel) of the chunk's slice read for every column point it feeds, and every V entry of
    rows 1-8 written once per board"""
    b2, vr = lay
    counts = [int((b2["item"][w, :, 0] >= 0).sum()) for w in range(8)]
    for w in range(8):
        assert (b2["item"][w, :counts[w]] >= 0).all() and (b2["item"][w, counts[w]:] == -1).all() and counts[w] <= 10
    assert len(set(counts[:4])) == 1 and len(set(counts[4:])) == 1 and counts[0] >= 4 and sum(counts) == 32
    seen = sorted((int(b), int(q)) for b, q in b2["item"].reshape(-1, 2) if b >= 0)
    assert seen == [(b, q) for b in range(2) for q in range(16)]
    r16, cb = int(vr["dims"][2]), int(vr["dims"][3])
    need = {(y * 8 + x, ch) for y in range(8) for x in range(8) for ch in range(32)}
    for b in range(2):
        got = set()
        for w in range(8):
            for k in range(8):
                if int(b2["item"][w, k, 0]) != b:
                    continue
                q = int(b2["item"][w, k, 1])
                for lane in range(64):
                    tc = lane >> 4
                    for j in range(4):
                        if (tc, j) in ((0, 0), (3, 3)):
                            continue                     # the clamped off-board column, multiplied by 0
                        sq, rem = divmod(int(vr["act"][q, lane, j]), r16)
                        got.add((sq, rem // cb))
        assert got == need, b


def test_global_offsets_stay_inside_the_workgroup(lay):
    """the four buffers tile the workgroup's bytes; the items' reads (every chunk) and the epilogue's 16-byte
    accesses stay inside a buffer, and the epilogue covers each (square, channel quad) once"""
    b2, vr = lay
    act, wg = int(b2["dims"][0]), int(b2["dims"][1])
    assert sorted(int(x) for x in b2["act"].ravel()) == [0, act, 2 * act, 3 * act] and 4 * act == wg
    assert int(b2["act"][0, 0]) == 0 and int(b2["act"][0, 1]) == act          # board 0: X, then H
    reads = vr["act"].astype(np.int64)[None] + 128 * np.arange(8)[:, None, None, None]
    assert reads.min() >= 0 and reads.max() + 4 <= act
    out = b2["out"].astype(np.int64)
    assert out.min() >= 0 and out.max() + 16 <= act and (out % 16 == 0).all()
    r16 = int(vr["dims"][2])
    cells = sorted((int(a) // r16, int(a) % r16 // 16) for a in out.ravel())
    assert cells == [(sq, quad) for sq in range(64) for quad in range(64)]
    for w in range(8):                                    # wave w owns channels 32 w .. 32 w + 31
        quads = {int(a) % r16 // 16 for a in out[w].ravel()}
        assert quads == set(range(8 * w, 8 * w + 8))


def test_lds_regions(lay):
    """the four V buffers are disjoint and fill the V region; the zero rows are 16 distinct runs in each
    buffer, none of them an entry an item writes; the ACT overlay lies inside V (live only while V is
    not), AUX lies behind V, and the total is within a CU's LDS"""
    b2, vr = lay
    act, wg, vbuf, ov_off, ov_bytes, aux_off, aux_bytes, lds = (int(x) for x in b2["dims"])
    starts = sorted(int(x) for x in b2["vbuf"].ravel())
    assert starts == [0, vbuf, 2 * vbuf, 3 * vbuf]
    assert int(b2["vbuf"][0, 1]) - int(b2["vbuf"][0, 0]) == vbuf           # a board's two buffers are adjacent
    vend = 4 * vbuf
    assert ov_off == 0 and ov_bytes == act and ov_off + ov_bytes <= vend
    assert aux_off == vend and aux_bytes >= 64 * 10 * 16 and aux_off + aux_bytes <= lds <= LDS_MAX
    zero = [int(z) for z in b2["zero"]]
    assert len(set(zero)) == 64 and all(z % 256 == 0 and 0 <= z and z + 256 <= vend for z in zero)
    written = {int(a) // 256 for a in vr["write"].ravel()}                  # runs an item writes, within a buffer
    for nb in range(2):
        for buf in range(2):
            base = int(b2["vbuf"][nb, buf])
            runs = {(z - base) // 256 for z in zero if base <= z < base + vbuf}
            assert len(runs) == 16 and not (runs & written)
            assert len(runs | written) == vbuf // 256                       # together they are the whole buffer
