"""
CPU tests of the rule by which sr_ct_palmer_sums_pack_f32_dev carries the next batch's pack inside the C(t) launch or launches kernel 0
in front of it: sr_ct_pack_fused(formulation, F, series, tiles, aligned) and the tile count sr_pack_reg_tiles(Npad, Vtot, v0, nV) it is
fed with (csrc/sr_ct.hip, csrc/sr_pack.hip) -- host functions that need no GPU, held against literals.
"""
import pytest

from spinrelax_amd import _lib

RFFT32, RFFT64, FFT64, DIRECT, BLOCKED = 4, 3, 2, 1, 5      # include/spinrelax_hip.h
NPAD = 100032                                               # 100 000 frames padded to a multiple of 64 (the pipelines' planes)


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def test_tiles_of_the_benchmark_shapes(lib):
    tiles = lib.sr_pack_reg_tiles
    assert tiles(NPAD, 512, 0, 512) == 782 * 16 == 12512                # cfg3
    assert tiles(NPAD, 2048, 0, 2048) == 782 * 64 == 50048              # cfg4
    assert tiles(NPAD, 512, 64, 64) == 782 * 2 == 1564                  # one of eight shards of cfg3
    assert tiles(8320, 32, 0, 32) == 65 and tiles(4224, 96, 32, 64) == 66 and tiles(128, 32, 0, 32) == 1 and tiles(4, 32, 0, 32) == 1
    # no whole 32-vector tiles, rows that are not 16 bytes, a first column that is not, Npad % 4, a range outside the array
    assert tiles(NPAD, 512, 0, 37) == 0 and tiles(NPAD, 33, 0, 32) == 0 and tiles(NPAD, 96, 1, 32) == 0
    assert tiles(NPAD + 2, 512, 0, 512) == 0 and tiles(NPAD, 512, 500, 32) == 0 and tiles(0, 512, 0, 512) == 0
    assert tiles(NPAD, 96, 4, 32) == 782                                # (v0 * 3) % 4 == 0


def test_the_launch_carries_the_pack_for_the_benchmark_shapes(lib):
    fused = lib.sr_ct_pack_fused
    assert fused(RFFT32, 4096, 24 * 512, 12512, 1) == 1                 # cfg3: 12 288 series, 224 workgroups take two tiles
    assert fused(RFFT32, 4096, 24 * 2048, 50048, 1) == 1                # cfg4
    assert fused(RFFT32, 4096, 24 * 64, 1564, 1) == 1                   # the 64-vector shard: 1 564 tiles for 1 536 series
    assert fused(RFFT32, 4096, 64, 33, 1) == 1 and fused(RFFT32, 4096, 64, 128, 1) == 1


def test_what_falls_back_to_kernel_0_in_front(lib):
    fused = lib.sr_ct_pack_fused
    assert fused(RFFT32, 4096, 64, 129, 1) == 0 and fused(RFFT32, 4096, 64, 195, 1) == 0      # more than two tiles per workgroup
    assert fused(RFFT32, 4096, 64, 0, 1) == 0                           # a shape without register tiles
    assert fused(RFFT32, 4096, 24 * 512, 12512, 0) == 0                 # a misaligned array of either job
    for form in (DIRECT, FFT64, RFFT64, BLOCKED, 0):
        assert fused(form, 4096, 24 * 512, 12512, 1) == 0               # only the float32 transforms have the carrying kernel
    for F in (1000, 2730, 4094, 4098, 5461):
        assert fused(RFFT32, F, 24 * 512, 12512, 1) == 0                # and only at the chunk length of cfg3 / cfg4
    assert fused(RFFT32, 4096, 0, 0, 1) == 0
