"""The synthetic day is an input of the benchmark and of the parity tests: the same arguments must
give the same day on every build.  Pins two generated days (messages, snapshots, snapshot indices)
by their SHA-256, recorded from the generator as it stood when the benchmark figures in BASELINE.md
were measured."""
import hashlib

import numpy as np
import pytest

from hftlob.data.synthetic import generate_day

DAYS = [(dict(n_msgs=20_000, seed=7, snap_every=6400),
         "ad39c88f938edabda6b521a970fd924e04bda9eae1b02882f838d5cbd5f772ed"),
        (dict(n_msgs=12_000, mid=28_000_000, tick=10, snap_every=100),
         "be93bfc32b59737b6c138bd604abd44f3f0acda064303b6ab550fd37f22fcf15")]


@pytest.mark.parametrize("kw,sha", DAYS, ids=["mid2m", "mid28m_tick10"])
def test_generated_day_is_pinned(kw, sha):
    d = generate_day(**kw)
    assert d.msgs.dtype == np.int32 and d.books.dtype == np.int32
    got = hashlib.sha256(d.msgs.tobytes() + d.books.tobytes() + d.snap_idx.astype(np.int64).tobytes()).hexdigest()
    assert got == sha
