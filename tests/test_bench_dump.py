"""CPU-only: bench.py --dump-outputs writes float32 / float64 .npy files within its byte budget, a larger output as a fixed, seeded row sample."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench      # noqa: E402


def test_dump_keeps_float32_and_writes_the_rest_as_float64(tmp_path):
  dth = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
  info = torch.tensor([0, 3], dtype=torch.int32)
  bench.dump_outputs(str(tmp_path), {'dtheta': dth, 'info': info})
  assert sorted(os.listdir(tmp_path)) == ['dtheta.npy', 'info.npy']
  a, i = np.load(tmp_path / 'dtheta.npy'), np.load(tmp_path / 'info.npy')
  assert a.dtype == np.float32 and np.array_equal(a, dth.numpy())
  assert i.dtype == np.float64 and np.array_equal(i, [0.0, 3.0])


def test_dump_over_budget_is_the_same_seeded_row_sample(tmp_path, monkeypatch):
  monkeypatch.setattr(bench, 'DUMP_BUDGET_BYTES', 4096)
  big = torch.arange(1000 * 8, dtype=torch.float32).reshape(1000, 8)
  err = torch.arange(1000, dtype=torch.float32)
  for d in ('a', 'b'):
    bench.dump_outputs(str(tmp_path / d), {'dtheta': big, 'err': err})
  total = sum(os.path.getsize(tmp_path / 'a' / f) for f in os.listdir(tmp_path / 'a'))
  assert total <= 4096 + 4 * 128      # (+ the .npy headers)
  rows = np.load(tmp_path / 'a' / 'dtheta_rows.npy')
  assert rows.dtype == np.float64 and np.array_equal(rows, np.load(tmp_path / 'a' / 'err_rows.npy'))
  assert np.array_equal(np.load(tmp_path / 'a' / 'dtheta.npy'), big.numpy()[rows.astype(np.int64)])
  assert np.array_equal(np.load(tmp_path / 'a' / 'err.npy'), err.numpy()[rows.astype(np.int64)])
  for f in os.listdir(tmp_path / 'a'):
    assert np.array_equal(np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f))
