"""The order in which the workgroups of a conv launch take its tiles (ddp_deal_tile of csrc/ddp_conv_deal.h, reached through the exported
host wrapper ddp_conv_deal_tile: the function the kernels call).  No GPU: the map is plain integer arithmetic."""
import ctypes as C

import numpy as np
import pytest

from diffdock_pocket_amd import _lib as L

CHUNKS = (4, 8, 16)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def deal_map(lib, total, c):
    return np.array([lib.ddp_conv_deal_tile(i, total, c) for i in range(total)], dtype=np.int64)


def range_order(total):
    """One contiguous range of tiles per XCD: the order of the launches before the chunks (written out here, not taken from the library)."""
    ids = np.arange(total, dtype=np.int64)
    q, rem, x = total >> 3, total & 7, ids & 7
    return np.where(x < rem, x * (q + 1), rem * (q + 1) + (x - rem) * q) + (ids >> 3)


@pytest.mark.parametrize("c", CHUNKS)
def test_bijection_for_every_total(lib, c):
    for total in range(1, 3001):
        m = deal_map(lib, total, c)
        assert np.array_equal(np.sort(m), np.arange(total)), (c, total)


def test_switch_zero_keeps_the_range_order(lib):
    for total in list(range(1, 300)) + [399, 512, 2938, 3000, 3191]:
        assert np.array_equal(deal_map(lib, total, 0), range_order(total)), total


@pytest.mark.parametrize("c", CHUNKS)
def test_small_launches_and_the_remainder_keep_the_range_order(lib, c):
    for total in range(1, 8 * c):
        assert np.array_equal(deal_map(lib, total, c), range_order(total)), (c, total)
    for total in (8 * c, 8 * c + 1, 24 * c + 13, 3191):
        whole = total - total % (8 * c)
        m = deal_map(lib, total, c)
        assert np.array_equal(np.sort(m[:whole]), np.arange(whole))
        assert np.array_equal(m[whole:], whole + range_order(total - whole)), (c, total)


@pytest.mark.parametrize("c", CHUNKS)
def test_chunks_are_runs_of_one_xcd(lib, c):
    """Inside the whole super-rows a chunk of c consecutive tiles belongs to ONE id class (XCD), in order; chunk m goes to XCD m % 8."""
    total = 3191
    m = deal_map(lib, total, c)
    xcd_of_tile = np.empty(total, dtype=np.int64)
    xcd_of_tile[m] = np.arange(total) & 7
    whole = total - total % (8 * c)
    chunks = xcd_of_tile[:whole].reshape(-1, c)
    assert np.all(chunks == chunks[:, :1])
    assert np.array_equal(chunks[:, 0], np.arange(whole // c) % 8)
    # and an XCD walks its tiles in ascending order
    for x in range(8):
        assert np.all(np.diff(m[x::8]) > 0)


@pytest.mark.parametrize("c", CHUNKS)
def test_every_xcd_receives_the_same_mix_of_tasks(lib, c):
    tiles = [1037, 726, 348, 726, 194, 160]      # six tasks of one launch, task-major
    total = sum(tiles)
    task_of_tile = np.repeat(np.arange(len(tiles)), tiles)
    m = deal_map(lib, total, c)
    for x in range(8):
        got = np.bincount(task_of_tile[m[x::8]], minlength=len(tiles))
        for i, n in enumerate(tiles):
            assert n // 8 - c <= got[i] <= -(-n // 8) + c, (c, x, i, int(got[i]), n)


def test_the_range_order_is_unbalanced_on_that_table(lib):
    """What the chunks are for: with one range per XCD some XCD holds no tile at all of the third task."""
    tiles = [1037, 726, 348, 726, 194, 160]
    task_of_tile = np.repeat(np.arange(len(tiles)), tiles)
    m = deal_map(lib, sum(tiles), 0)
    per_xcd = np.array([np.bincount(task_of_tile[m[x::8]], minlength=len(tiles))[2] for x in range(8)])
    assert per_xcd.min() == 0 and per_xcd.max() > 348 // 2


def test_arguments_out_of_range(lib):
    for id_, total, c in ((-1, 10, 8), (10, 10, 8), (0, 0, 8), (0, 10, -1), (0, 10, 4097)):
        assert lib.ddp_conv_deal_tile(id_, total, c) == -1


def test_the_switch_is_an_exported_int(lib):
    v = C.c_int.in_dll(lib, "ddp_conv_deal")
    assert -1 <= v.value <= 4096
