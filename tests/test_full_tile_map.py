"""CPU checks of the FULL-packet placement helpers of libroxtrace.so: the workgroup -> tile map
(rox_args.hpp full_tile_map(), through rox_diag_full_tile_map) is a bijection of [0, n_tiles)
for every group size and grid, and rox_packet_ld keeps its footprint cap.  No device needed."""
import ctypes as C
import os

import numpy as np
import pytest

from rayoptics_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_TILES = (1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 257, 1024, 1031)
GROUPS = (0, 1, 2, 4, 8, 16, 32)


@pytest.fixture(scope='module')
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        'rox_build', os.path.join(ROOT, 'ray-optics_amd', 'build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return abi.declare(C.CDLL(b.build()))


def tile_map(lib, n_tiles, group, grid, wg0=0):
    tiles = np.full(n_tiles, -1, dtype=np.int64)
    rc = lib.rox_diag_full_tile_map(n_tiles, group, grid, wg0,
                                    tiles.ctypes.data_as(C.POINTER(C.c_int64)))
    assert rc == 0, lib.rox_last_error()
    return tiles


def grids_of(n_tiles):
    """the whole launch in one pass, and grids the walk strides over: a multiple of the XCD
    count, one that is not, a single workgroup"""
    return sorted({g for g in (n_tiles, n_tiles - 1, n_tiles // 2, 8, 5, 1) if 1 <= g <= n_tiles})


@pytest.mark.parametrize('group', GROUPS)
@pytest.mark.parametrize('n_tiles', N_TILES)
def test_tile_map_is_a_bijection(lib, n_tiles, group):
    for grid in grids_of(n_tiles):
        for wg0 in (0, 3, grid):          # item 0; an item whose first workgroup is on another XCD
            tiles = tile_map(lib, n_tiles, group, grid, wg0)
            assert np.array_equal(np.sort(tiles), np.arange(n_tiles)), (n_tiles, group, grid, wg0)


@pytest.mark.parametrize('n_tiles', N_TILES)
def test_group_zero_and_the_ragged_remainder_are_the_identity(lib, n_tiles):
    assert np.array_equal(tile_map(lib, n_tiles, 0, n_tiles), np.arange(n_tiles))
    for group in GROUPS[1:]:
        whole = n_tiles // (8 * group) * (8 * group)
        tiles = tile_map(lib, n_tiles, group, n_tiles)
        assert np.array_equal(tiles[whole:], np.arange(whole, n_tiles))
        # a block's tiles stay in the block
        assert np.array_equal(tiles[:whole] // (8 * group), np.arange(whole) // (8 * group))


def test_an_xcd_gets_contiguous_runs(lib):
    """130 tiles, 16 per run: workgroups 8 apart (one XCD) walk tiles 16 x .. 16 x + 15 of the one
    whole block; tiles 128, 129 stay"""
    tiles = tile_map(lib, 130, 16, 130)
    for x in range(8):
        assert np.array_equal(tiles[x:128:8], np.arange(16 * x, 16 * x + 16))
    assert list(tiles[128:]) == [128, 129]
    # the second item of a batched launch of 130-workgroup items starts on XCD 130 % 8 = 2
    shifted = tile_map(lib, 130, 16, 130, wg0=130)
    for x in range(8):
        assert np.array_equal(shifted[(x - 2) % 8:128:8], np.arange(16 * x, 16 * x + 16))


def test_tile_map_rejects_bad_arguments(lib):
    buf = (C.c_int64 * 4)()
    assert lib.rox_diag_full_tile_map(4, -1, 4, 0, buf) == -1
    assert lib.rox_diag_full_tile_map(4, 1, 0, 0, buf) == -1
    assert lib.rox_diag_full_tile_map(-1, 1, 4, 0, buf) == -1
    assert lib.rox_diag_full_tile_map(4, 1, 4, 0, None) == -1


@pytest.mark.parametrize('R', (1, 63, 4096, 2 ** 20, 2 ** 28))
def test_packet_ld_is_at_least_the_rays_and_keeps_the_pad_cap(lib, R):
    ld = lib.rox_packet_ld(R)
    assert ld >= R
    assert ld - R <= max(256, R // 16)


def test_packet_ld_rows_are_whole_cache_lines_and_never_a_power_of_two_apart(lib):
    for R in (1, 45 * 46, 4096, 10000, 364 * 364, 2 ** 20, 2 ** 20 + 1, 2 ** 28):
        ld = lib.rox_packet_ld(R)
        assert R <= ld <= R + max(256, R // 16) and ld % 8 == 0, R
        if R >= 4096:
            assert ld & (ld - 1), R
    assert lib.rox_packet_ld(0) == 1 and lib.rox_packet_ld(-5) == 1


def test_engine_pitch_is_the_library_s(lib):
    from rayoptics_amd.engine import padded_ld
    for R in (1, 63, 2070, 4096, 2 ** 20):
        assert padded_ld(R) == lib.rox_packet_ld(R)
