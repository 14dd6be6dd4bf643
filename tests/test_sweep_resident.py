"""The sweep megakernel's two-barrier form: resident state, folded reduce,
parity slots and the monotonic barrier (eagle_sweep.hip).

Every comparison is BITWISE, on `pool_cont`, `rewards`, `perts`, `best` and
`iter_t[:2]`, against the standalone step kernels
(`sweep_cases.compose_step_kernels`) or against the same iterations cut into
several `ext.eagle_sweep` calls. Every call gets a zeroed barrier buffer:
the barrier counts arrivals upwards from zero over one launch.

  mode boundary     pool * dc = 4096 keeps the state in LDS for the whole
                    launch and takes no barrier after the update; 4224
                    takes the legacy path (state in global memory, pool
                    staged per iteration, C-to-A barrier)
  reduce threshold  1024 tile partials are reduced inside the update phase;
                    1089 keep phase B2 and its barrier
  hand-over         the resident state is loaded at the start of a launch
                    and stored at its end: one call == many calls
  parity slots      a single batch rewrites the same fireflies every
                    iteration, so a candidate read from the wrong slot
                    changes the result
  many barriers     2000 iterations in one launch: 4000 generations of the
                    counter
"""

import dataclasses

import numpy as np
import pytest
import torch

import sweep_cases as sw

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


def _case(shape, name):
  pool, batch, dc, n = shape
  return sw.make_sweep_case(pool, batch, dc, n, seed=pool + 3 * dc + n,
                            name=name)


def _assert_state_equal(got, want, tag):
  for key in ('pool_cont', 'rewards', 'perts', 'best'):
    assert torch.equal(getattr(got, key), getattr(want, key)), (tag, key)
  assert got.iter_t[:2].tolist() == want.iter_t[:2].tolist(), tag


def _run_split(ext, case, chunks):
  """The iterations of `chunks`, one `ext.eagle_sweep` call per chunk on
  the same state tensors, `it_start` advancing, a zeroed barrier each."""
  call = sw.sweep_call(case, chunks[0])
  done = 0
  for its in chunks:
    step = dataclasses.replace(
        call, it_start=case.it_start + done, iterations=its,
        barrier=torch.zeros_like(call.barrier))
    ext.eagle_sweep(*step.args())
    done += its
  torch.cuda.synchronize()
  return call


# -- 1. mode boundary -----------------------------------------------------------------

BOUNDARY = {
    'resident-4096': (128, 32, 32, 130),
    'legacy-4224': (128, 32, 33, 130),
}


@pytest.mark.parametrize('name', BOUNDARY)
def test_mode_boundary_equals_step_kernels(ext, name):
  case = _case(BOUNDARY[name], name)
  assert (case.pool * case.dc <= 4096) == (name == 'resident-4096')
  its = case.full_iterations()
  got = sw.run_sweep(ext, case, its)
  want = sw.compose_step_kernels(ext, case, its)
  _assert_state_equal(got, want, name)
  assert not torch.equal(got.pool_cont.cpu(),
                         torch.from_numpy(case.pool_cont))


# -- 2. reduce threshold --------------------------------------------------------------

THRESHOLD = {
    'folded-1024': (50, 25, 3, 2048),
    'b2-1089': (50, 25, 3, 2049),
}


@pytest.mark.parametrize('name', THRESHOLD)
def test_reduce_threshold_equals_step_kernels(ext, name):
  """`compose_step_kernels` does not expose the step path's reduced
  quadform, so `var_ws[:, T]` is held to the fp64 sum of the kernel's own
  partials within T 2^-24 sum|partials|, as test_sweep_kernel.py does; the
  bitwise check of the reduce order is the state comparison."""
  case = _case(THRESHOLD[name], name)
  assert case.tiles == (1024 if name == 'folded-1024' else 1089)
  got = sw.run_sweep(ext, case, 3)
  want = sw.compose_step_kernels(ext, case, 3)
  _assert_state_equal(got, want, name)
  T = case.tiles
  var = got.var_ws.cpu().double()
  parts = var[:, :T]
  err = (var[:, T] - parts.sum(1)).abs()
  tol = T * EPS * parts.abs().sum(1)
  worst = int(torch.argmax(err - tol))
  print(f'OBSERVED {name} reduce of {T} tiles: err {float(err[worst]):.3e} '
        f'(bound {float(tol[worst]):.3e})')
  assert bool((err <= tol).all()), name     # NaN partials fail here


# -- 3. state hand-over through global memory ---------------------------------------------


@pytest.mark.parametrize('case_id', ('base', 'max-batch'))
def test_split_calls_equal_one_call(ext, case_id):
  case = sw.case_by_id(case_id)
  assert case.pool * case.dc <= 4096      # resident
  its = case.full_iterations()
  whole = sw.run_sweep(ext, case, its)
  _assert_state_equal(whole, sw.compose_step_kernels(ext, case, its),
                      case_id)
  for chunks in ([1] * its, [2, its - 2]):
    split = _run_split(ext, case, chunks)
    _assert_state_equal(split, whole, (case_id, chunks))


# -- 4. parity slots ------------------------------------------------------------------------


def test_single_batch_parity_slots(ext):
  case = sw.case_by_id('single-batch')
  assert case.n_batches == 1
  got = sw.run_sweep(ext, case, 6)
  want = sw.compose_step_kernels(ext, case, 6)
  _assert_state_equal(got, want, 'single-batch x 6')
  assert want.dead >= 1


# -- 5. many barriers -------------------------------------------------------------------------


def test_two_thousand_iterations_in_one_launch(ext):
  case = sw.case_by_id('b1')
  whole = sw.run_sweep(ext, case, 2000)
  split = _run_split(ext, case, [1000, 1000])
  _assert_state_equal(split, whole, 'b1 x 2000')
  assert np.isfinite(whole.pool_cont.cpu().numpy()).all()
