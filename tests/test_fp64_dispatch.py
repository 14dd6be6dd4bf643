"""CPU side of the fp64 HIP path: the opt-in flag, the dispatch rules that
must NOT change for CPU tensors, the megakernel dtype gate, and the NumPy
splitmix64 oracle the GPU tests (test_fp64_kernels.py) rely on."""

import types

import numpy as np
import torch

import eagle_f64_oracle as oracle
from vizier_amd._src.algorithms.optimizers import eagle as eagle_lib
from vizier_amd._src.algorithms.optimizers import vectorized
from vizier_amd._src.gp import matern
from vizier_amd._src.ops import dispatch


def test_flag_follows_env_at_call_time(monkeypatch):
  monkeypatch.delenv('VIZIER_AMD_FP64_HIP', raising=False)
  assert dispatch.fp64_hip_enabled() is False
  monkeypatch.setenv('VIZIER_AMD_FP64_HIP', '1')
  assert dispatch.fp64_hip_enabled() is True
  for other in ('0', '', 'true', '11'):
    monkeypatch.setenv('VIZIER_AMD_FP64_HIP', other)
    assert dispatch.fp64_hip_enabled() is False
  monkeypatch.setenv('VIZIER_AMD_FP64_HIP', '1')
  assert dispatch.fp64_hip_enabled() is True
  monkeypatch.delenv('VIZIER_AMD_FP64_HIP')
  assert dispatch.fp64_hip_enabled() is False


def test_cpu_float64_keeps_the_torch_path(monkeypatch):
  g = torch.Generator().manual_seed(0)
  x1 = torch.rand(37, 5, generator=g, dtype=torch.float64)
  x2 = torch.rand(11, 5, generator=g, dtype=torch.float64)
  ls = 0.5 + torch.rand(5, generator=g, dtype=torch.float64)
  amp = torch.tensor(1.3, dtype=torch.float64)
  want_cross = matern.gram_matern52(x1, x2, ls, amp)
  want_self = matern.gram_matern52(x1, None, ls, amp)
  monkeypatch.delenv('VIZIER_AMD_FP64_HIP', raising=False)
  off = (dispatch.gram_matern52(x1, x2, ls, amp),
         dispatch.gram_matern52(x1, None, ls, amp))
  monkeypatch.setenv('VIZIER_AMD_FP64_HIP', '1')
  assert not dispatch.use_fp64_hip(x1)
  on = (dispatch.gram_matern52(x1, x2, ls, amp),
        dispatch.gram_matern52(x1, None, ls, amp))
  for got in (off, on):
    assert torch.equal(got[0], want_cross)
    assert torch.equal(got[1], want_self)


def test_cpu_float64_strategy_has_no_extension(monkeypatch):
  monkeypatch.setenv('VIZIER_AMD_FP64_HIP', '1')
  strategy = eagle_lib.VectorizedEagleStrategy(
      n_continuous=3, categorical_sizes=[], device='cpu',
      dtype=torch.float64)
  assert strategy._ext is None


def _megakernel_stub(dtype):
  """Everything _megakernel_applicable looks at, satisfied, but `dtype`."""
  x = types.SimpleNamespace(is_cuda=True, shape=(64, 4))
  scoring = types.SimpleNamespace(
      posterior=types.SimpleNamespace(K_inv=object(), x=x),
      _acq_name='ucb', _tr_anchored=True, gram_dtype='fp32')
  strategy = types.SimpleNamespace(
      _ext=object(), categorical_sizes=[], n_parallel=1, pool_size=50,
      batch_size=25, dtype=dtype)
  score_fn = types.SimpleNamespace(scoring=scoring, codec_identity=True)
  return vectorized.VectorizedOptimizer(strategy), score_fn


def test_megakernel_is_fp32_only(monkeypatch):
  monkeypatch.delenv('VIZIER_AMD_MEGAKERNEL', raising=False)
  opt, score_fn = _megakernel_stub(torch.float32)
  assert opt._megakernel_applicable(score_fn)
  opt, score_fn = _megakernel_stub(torch.float64)
  assert not opt._megakernel_applicable(score_fn)


def test_splitmix64_oracle_known_values():
  # vz_splitmix64(z) = mix(z + 0x9e3779b97f4a7c15) with the multipliers
  # 0xbf58476d1ce4e5b9 / 0x94d049bb133111eb and shifts 30 / 27 / 31 of
  # common.h. By hand for z = 0: z + golden = 0x9e3779b97f4a7c15, and the
  # two xor-shift-multiply rounds and the final xor-shift give
  # 0xe220a8397b1dcdaf; z = golden and z = 2 * golden (mod 2^64) are the
  # next two states of the same sequence.
  golden = 0x9e3779b97f4a7c15
  got = oracle.splitmix64(np.array(
      [0, golden, (2 * golden) % 2**64], dtype=np.uint64))
  assert [int(v) for v in got] == [
      0xe220a8397b1dcdaf, 0x6e789e6aa1b965f4, 0x06c45d188009454f]
  # The uniform keeps the top 24 bits: ((h >> 40) + 0.5) / 2^24.
  h = int(oracle.splitmix64(7 ^ int(oracle.splitmix64(3 ^ 5))))
  assert float(oracle.uniform(7, 3, 5)) == ((h >> 40) + 0.5) / 2.0**24
