"""bench.py's command line: --full and --dump-outputs exist, and --dump-outputs writes what the
timed call returned and left behind as float arrays, the same from run to run."""
import os
import subprocess
import sys

import numpy as np

from bpe_amd import ROOT

BENCH = os.path.join(ROOT, 'bench.py')


def test_options_exist():
    usage = subprocess.run([sys.executable, BENCH, '--help'], capture_output=True, text=True,
                           cwd=ROOT).stdout
    assert '--full' in usage and '--dump-outputs' in usage


def test_dump_outputs_writes_float_arrays(tmp_path):
    import bench

    class Engine:
        def sample_lengths(self):
            return np.arange(10, 20, dtype=np.int64)

        def read_samples(self, idx):
            off = np.concatenate([[0], np.cumsum(self.sample_lengths()[idx])]).astype(np.int64)
            return np.arange(off[-1], dtype=np.int32), off

    class Trainer:
        engine = Engine()

    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), Trainer(), [(1, 2, 30), (4, 5, 6)])
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['merges.npy', 'sample_ids.npy', 'sample_index.npy', 'sample_lengths.npy',
                     'sample_offsets.npy']
    for n in names:
        a, b = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
    assert np.load(tmp_path / 'a' / 'merges.npy').tolist() == [[1, 2, 30], [4, 5, 6]]
    idx = np.load(tmp_path / 'a' / 'sample_index.npy')
    assert len(idx) == bench.DUMP_SAMPLES and len(set(idx.tolist())) == len(idx)
