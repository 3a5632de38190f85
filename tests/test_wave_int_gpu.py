"""csrc/wave_int.h on the device, function by function (se2gpu_debug_wave_int: one workgroup of 64, 256 or 1024 threads walks n values
in chunks of its size), against numpy, for exact equality: the integer wave sum / minimum / maximum, the wave inclusive scan, the
ballot rank and the workgroup exclusive scan - looped over the chunks on the same words of LDS with a running total, and on one
chunk without the barrier in front of the LDS write - as int and as long long.  The sizes sit on both sides of a wave, of every
workgroup size and of two chunks of the largest; the long long data does not fit 32 bits after a few additions."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
BLOCKS = (64, 256, 1024)


def _data(n, kinds):
    rng = np.random.default_rng(1000 + n)
    every = {"zeros": np.zeros(n, np.int64), "ones": np.ones(n, np.int64), "pos": rng.integers(0, 1001, n),
             "signed": rng.integers(-1000, 1001, n), "bits": rng.integers(0, 2, n),
             "big": (1 << 40) + rng.integers(-(1 << 20), 1 << 20, n)}
    return [(k, every[k].astype(np.int64)) for k in kinds]


def _device(op, block, x):
    from se2lam_amd import capi
    return capi.debug_wave_int(op, block, x)


def _wave_starts(n):
    return np.arange(0, n, 64)


def _per_wave(x, ufunc):
    """ufunc over every 64 consecutive values, repeated for each of them"""
    starts = _wave_starts(len(x))
    return np.repeat(ufunc.reduceat(x, starts), np.diff(np.append(starts, len(x))))


def _wave_scan(x):
    """inclusive prefix sum that restarts every 64 values"""
    c = np.cumsum(x)
    starts = _wave_starts(len(x))
    before = np.where(starts > 0, c[starts - 1], 0)
    return c - np.repeat(before, np.diff(np.append(starts, len(x))))


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("op,ufunc", [("sum", np.add), ("min", np.minimum), ("max", np.maximum)])
def test_wave_sum_min_max(op, ufunc, block):
    for n in SIZES:
        for name, x in _data(n, ("zeros", "ones", "pos", "signed")):
            got = _device(op, block, x)
            assert np.array_equal(got, _per_wave(x, ufunc)), (op, block, n, name)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("op,kinds", [("scan_i32", ("zeros", "ones", "pos", "signed")), ("scan_i64", ("zeros", "ones", "pos", "big"))])
def test_wave_scan_incl(op, kinds, block):
    for n in SIZES:
        for name, x in _data(n, kinds):
            got = _device(op, block, x)
            assert np.array_equal(got, _wave_scan(x)), (op, block, n, name)


@pytest.mark.parametrize("block", BLOCKS)
def test_lane_rank(block):
    for n in SIZES:
        for name, x in _data(n, ("zeros", "ones", "pos", "bits")):
            set_ = (x != 0).astype(np.int64)
            got = _device("rank", block, x)
            assert np.array_equal(got, _wave_scan(set_) - set_), (block, n, name)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("op,kinds", [("block_scan_i32", ("zeros", "ones", "pos", "signed")),
                                      ("block_scan_i64", ("zeros", "ones", "pos", "big"))])
def test_block_scan_excl_looped(op, kinds, block):
    """n > block: the second and later chunks write s_w while a slower wave may still read the round before"""
    for n in SIZES:
        for name, x in _data(n, kinds):
            got = _device(op, block, x)
            want = np.append(np.cumsum(x) - x, x.sum())
            assert np.array_equal(got, want), (op, block, n, name)
    if op == "block_scan_i64":
        assert _data(SIZES[-1], ("big",))[0][1].sum() > 1 << 32       # the data is what the docstring says


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("op,kinds", [("fresh_scan_i32", ("zeros", "ones", "pos", "signed")),
                                      ("fresh_scan_i64", ("zeros", "ones", "pos", "big"))])
def test_block_scan_excl_fresh(op, kinds, block):
    for n in [s for s in SIZES if s <= block]:
        for name, x in _data(n, kinds):
            got = _device(op, block, x)
            want = np.append(np.cumsum(x) - x, x.sum())
            assert np.array_equal(got, want), (op, block, n, name)


def test_arguments_are_checked():
    from se2lam_amd import capi
    x = np.ones(65, np.int64)
    with pytest.raises(capi.Se2GpuError):
        _device("sum", 128, x)                                         # a workgroup size the entry does not have
    with pytest.raises(capi.Se2GpuError):
        _device("fresh_scan_i32", 64, x)                               # more than one chunk
