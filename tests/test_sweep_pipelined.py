"""The sweep megakernel's loops with their loads in flight (eagle_sweep.hip):
the batched staging of k_i / k_j in the sweep's own tile routine, and the
k-vector over four rows and chunks of four dimensions.

Every comparison is BITWISE, on `pool_cont`, `rewards`, `perts`, `best` and
`iter_t[:2]`, against the standalone step kernels
(`sweep_cases.compose_step_kernels`), which keep the rolled loops and the
shared `vz_quadform_tile`. Every case runs `full_iterations()`: each batch
is visited twice. Default grid.

One axis varies per case, the others stay small (`(pool, batch, dc, n)`):

  dc     1, 3 scalar form below one chunk; 4 one float4 chunk exactly; 5 a
         chunk plus a tail (scalar form); 8 two float4 chunks; 20 the
         headline; 21 its scalar neighbour
  n      3 a partial tile with fewer rows than a wave has lanes; 63 / 64 /
         65 around the tile; 129 a third tile; 257 one row in a thread's
         second slot of the four-row trip; 1025 one row in the second trip
  pool   7, 26, 100 (the headline), 128 (MAX_POOL)
  batch  1, 7, 25, 32 (VZ_QF_QMAX: every staging row of a thread live)
  mode   legacy with the pool staged per iteration, and with the pool read
         through memory-side loads

The pool sizes and the two legacy modes bracket a chunked form of the
suggest step's loops (16 fireflies, 8 dimensions per chunk) that was
measured and left out (profiles/bench_sweep_loads_in_flight.md); they stay
so that a later attempt meets them.

`make_sweep_case` wants `pool % batch == 0`, so pool 7 runs as one batch of
7 (which is also the batch-7 case), pool 26 as batches of 2, and batch 25
on a pool of 50. It accepts every shape of the list, n = 3 included.
"""

import pytest
import torch

import sweep_cases as sw

pytestmark = pytest.mark.gpu

SMALL = dict(pool=8, batch=4, dc=4, n=70)


def _shape(**kw):
  s = dict(SMALL, **kw)
  return (s['pool'], s['batch'], s['dc'], s['n'])


CASES = {}
for _dc in (1, 3, 4, 5, 8, 20, 21):
  CASES[f'dc-{_dc}'] = _shape(dc=_dc)
for _n in (3, 63, 64, 65, 129, 257, 1025):
  CASES[f'n-{_n}'] = _shape(n=_n)
CASES.update({
    'pool-7-batch-7': _shape(pool=7, batch=7, dc=5),
    'pool-26': _shape(pool=26, batch=2, dc=5),
    'pool-100': _shape(pool=100, batch=4, dc=5),
    'pool-128': _shape(pool=128, batch=4, dc=5),
    'batch-1': _shape(pool=8, batch=1),
    'batch-25': _shape(pool=50, batch=25),
    'batch-32': _shape(pool=64, batch=32),
    'legacy-staged': (128, 32, 33, 130),
    'legacy-unstaged': (128, 32, 65, 70),
})


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


@pytest.mark.parametrize('name', CASES)
def test_pipelined_sweep_equals_step_kernels(ext, name):
  pool, batch, dc, n = CASES[name]
  case = sw.make_sweep_case(pool, batch, dc, n, seed=pool + 3 * dc + n,
                            name=name)
  if name == 'legacy-staged':
    assert 4096 < pool * dc <= 8192
  if name == 'legacy-unstaged':
    assert pool * dc > 8192
  its = case.full_iterations()
  got = sw.run_sweep(ext, case, its)
  want = sw.compose_step_kernels(ext, case, its)
  for key in ('pool_cont', 'rewards', 'perts', 'best'):
    assert torch.equal(getattr(got, key), getattr(want, key)), (name, key)
  assert got.iter_t[:2].tolist() == want.iter_t[:2].tolist(), name
  assert not torch.equal(got.pool_cont.cpu(),
                         torch.from_numpy(case.pool_cont))
