"""
CPU tests of the fused chunk statistics (GroupedPipeline's `fused_stats`): what the two new entry points refuse without a context, the
footprint of the raw sums a group keeps and the rule by which the pipeline falls back to the per-batch launches -- host functions that
need no GPU, held against literals.  (The refusals that need a context, -2 and -3, are asserted in tests/test_gpu_fused_stats.py and
tests/test_gpu_transpose_batched.py.)
"""
import pytest

from spinrelax_amd import _lib
from spinrelax_amd import pipeline as pl


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def test_no_context_is_refused_on_the_host(lib):
    # no context: refused on the host, nothing touched
    assert lib.sr_transpose_batched_f64_dev(None, None, 1, 1, 1, None) == -1
    assert lib.sr_expfit_order_search_sums_f64_dev(None, None, 1, None, 1, 2, None, None, 1, 1, None, 1, None, 1, 1.0, 0.5, None, None, 0,
                                                   None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert b'null sr_ctx' in lib.sr_last_error()


def test_raw_sum_row_of_the_benchmark_shape(lib):
    # lags 0 .. 2048 and the slack of the direct kernel's last 128-lag block, rounded up to 8 doubles
    assert lib.sr_ct_psum_stride(4096) == 2184
    assert lib.sr_ct_psum_stride(512) == 392 and lib.sr_ct_psum_stride(20) == 144


def test_footprint_of_the_group_tensors():
    # cfg3: 512 vectors, 24 chunks of 4096 frames, groups of 32 -- two group buffers
    assert pl.fused_stats_bytes(32, 512, 24, 2184) == 13740539904                  # 13.7 GB (12.9 GB of them are ever read: L of Lp slots)
    assert pl.fused_stats_bytes(32, 512, 24, 2184) == 2 * 32 * 214695936           # a batch's raw sums: 214.7 MB
    assert pl.fused_stats_bytes(20, 512, 24, 2184) == 8587837440                   # groups of 20
    assert pl.fused_stats_bytes(2, 8, 3, 392) == 301056                            # the pipeline test's shape
    assert pl.fused_stats_bytes(1, 1, 1, 8) == 128


def test_fallback_rule_half_of_the_free_memory():
    need = pl.fused_stats_bytes(32, 512, 24, 2184)
    assert pl.fused_stats_fits(need, 288 * 10 ** 9)                                # an idle MI355X
    assert pl.fused_stats_fits(need, 2 * need) and pl.fused_stats_fits(need, 2 * need + 1)
    assert not pl.fused_stats_fits(need, 2 * need - 1)                             # more than half of what is free: per-batch launches
    assert not pl.fused_stats_fits(need, 16 * 10 ** 9) and not pl.fused_stats_fits(1, 0)
    assert pl.fused_stats_fits(0, 0)


def test_default_is_on():
    assert pl.FUSED_STATS_DEFAULT is True
