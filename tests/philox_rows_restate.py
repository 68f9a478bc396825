"""Row addressing of the seeded noise generator (switch_nerf_amd/csrc/rng.hip swn_rng_fill_rows), restated over tests/philox_restate.py:
output row j holds the per_row elements from (row_base + row_index[j]) * per_row on, of (seed, step, stream, domain); the domain enters
the generator as bits 8.. of the counter word that carries the stream id.  Shared by tests/test_bg_device_noise_cpu.py and
tests/test_bg_device_noise_gpu.py."""
import numpy as np

import philox_restate as R


def counter_word(stream: int, domain: int) -> int:
    return stream | (domain << 8)


def _rows(row_index, n_rows):
    return range(n_rows) if row_index is None else [int(i) for i in row_index]


def uniform_rows(seed, step, stream, domain, row_base, row_index, per_row, n_rows=None):
    """float32 [n_rows, per_row], compared bit for bit; row_index None = the identity over n_rows rows."""
    w = counter_word(stream, domain)
    return np.stack([R.uniform(seed, step, w, (row_base + i) * per_row, per_row) for i in _rows(row_index, n_rows)])


def normal_rows(seed, step, stream, domain, row_base, row_index, per_row, n_rows=None, scale=1.0):
    """float64 [n_rows, per_row]: each row is a run of the GLOBAL normal sequence, so a row that starts on an odd element begins with the
    sin half of the Box-Muller pair it shares with the element before it (philox_restate.normal handles the odd base)."""
    w = counter_word(stream, domain)
    return np.stack([R.normal(seed, step, w, (row_base + i) * per_row, per_row, scale=scale) for i in _rows(row_index, n_rows)])
