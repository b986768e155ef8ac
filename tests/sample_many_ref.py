"""The cases of the batched soft_measure (include/qip_hipx.h) and a vectorised form of measure_ref.crossing_ref — shared by
tests/test_hipx_contract_cpu.py and tests/test_gpu_f1_sample_many.py.  A plain helper module: numpy only, no fixtures."""
import numpy as np

import measure_ref as R

# (B): a sample is compared with the exact crossing only when it is farther than the margin from every partial sum.
#   f64: the device sums at most 2^16 products <= 1 in double, an error below 2^16 * 2^-53 ~ 7e-12; 1e-9 is also the kernels'
#        own skip margin.
#   f32: the sample is rounded to f32 first; measure_ref.SOFT_MARGIN (the f32 replay of the crossing sub-range).
# (dtype, n, count, margin)
MARGIN_CASES = tuple((np.complex128, n, 4096, 1e-9) for n in (10, 12, 14, 16)) + tuple(
    (np.complex64, n, 1024, R.SOFT_MARGIN) for n in (6, 10))


def samples(n, count):
    return np.random.default_rng(7000 + n).uniform(0, 1, count)


def margin_samples(dtype, n, count):
    rs = samples(n, count)
    return rs.astype(np.float32).astype(np.float64) if dtype == np.complex64 else rs


def crossing_many(x, rs):
    """measure_ref.crossing_ref for an array of samples: (int64[len(rs)] first index at which the running sum of the products
    reaches the sample, 0 when it never does; float64[len(rs)] distance from the sample to the nearest partial sum)"""
    cum = np.cumsum(R.products(x), dtype=np.longdouble)
    rs = np.asarray(rs, dtype=np.longdouble)
    at = np.searchsorted(cum, rs, side="left")  # the first i with cum[i] >= r, i.e. r - cum[i] <= 0
    last = len(cum) - 1
    above = np.abs(cum[np.minimum(at, last)] - rs)
    below = np.abs(cum[np.clip(at - 1, 0, last)] - rs)  # (at = 0: cum[0] again, the sum above)
    return np.where(at <= last, at, 0).astype(np.int64), np.minimum(above, below).astype(np.float64)
