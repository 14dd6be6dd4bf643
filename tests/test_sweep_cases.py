"""CPU self-check of tests/sweep_cases.py: the INPUTS of the sweep
megakernel tests are what they claim, established with the oracle alone.

"Candidates" here are `oracle.suggest` evaluated in fp32 arithmetic; the
GPU test repeats the kind and margin checks on the kernel's own candidates.
"""

import types

import numpy as np
import pytest
import torch

import scorer_cases as sc
import sweep_cases as sw

ALL_IDS = (list(sw.CASES) + [f'{name}-tr' for name in sw.TR_CASES] +
           ['base-newbest'])
TR_SETTINGS = (sc.TR_RADIUS, 0.0, 0.6)


def _observed(case):
  return types.SimpleNamespace(out_cont=sw.oracle_candidates(case, sw.F32))


def _settings(case):
  """(acq, tr_radius) pairs the GPU tests run on this case."""
  acqs = sc.ACQ_NAMES if case.name in sw.ACQ_CASES else ['ucb']
  radii = TR_SETTINGS if case.tr else (0.0,)
  return [(acq, r) for acq in acqs for r in radii]


@pytest.mark.parametrize('case_id', ALL_IDS)
def test_roles_are_reached_with_margin(case_id):
  case = sw.case_by_id(case_id)
  visited = slice(case.start, case.start + case.batch)
  assert case.start > 0 or case.n_batches == 1
  assert int(np.isinf(case.rewards).sum()) == 3
  n_inside = int(np.isinf(case.rewards[visited]).sum())
  assert case.roles.count('ninf') == n_inside
  if case.n_batches > 1:
    assert n_inside < 3                       # s = 0 for a non-finite row
  if case.batch >= 4:
    assert n_inside >= 1                      # my_reward = -inf
  full = case.batch >= sw.FULL_ROLES_BATCH and case_id != 'base-newbest'
  if full:
    assert case.roles.count('low') >= 2
    assert case.roles.count('high') >= 2
    assert case.roles.count('dead') >= 2
    assert case.roles.count('best') == 1
  lb, pf = 7e-5, 0.7
  for i, role in enumerate(case.roles):
    if role in ('dead', 'best'):
      assert lb <= case.perts[case.start + i] < lb / pf
  want_kind = {'low': 'improved', 'ninf': 'improved', 'high': 'penalised',
               'best': 'penalised', 'dead': 'dead'}

  observed = _observed(case)
  for acq, tr_radius in _settings(case):
    o64 = sw.oracle_iteration(case, acq, sc.COEF, sw.BEST_VALUE, tr_radius,
                              observed)
    o32 = sw.oracle_iteration(case, acq, sc.COEF, sw.BEST_VALUE, tr_radius,
                              observed, dtype=torch.float32)
    # No row within tolerance of its threshold: fp32 and fp64 scores of the
    # same candidates give every row the same kind, the one its role names.
    assert o64.kinds == o32.kinds == [want_kind[r] for r in case.roles]
    assert sw.observed_kinds(case, o64.rewards, o64.perts) == o64.kinds
    # The tolerances of scorer_cases are worked out for sd ~ 0.7 amp
    # (max quad = 0.5 amp^2 on make_case's own xq). The sweep's candidates
    # are other points of the same cube: the quadform stays that size.
    assert 0.65 * sc.AMP <= float(o64.sd.min()), float(o64.sd.min())
    assert float(o64.quad.min()) > 0.0
    # "Far": further than 100 x the score tolerance from the score range.
    code = sc.ACQ_NAMES.index(acq)
    tol = sc.TOL_PENALTY if bool(o64.penalised.any()) else \
        sc.acq_tolerance(code)
    lo, hi = float(o64.score.min()), float(o64.score.max())
    adjusted = case.rewards[visited][np.isfinite(case.rewards[visited])]
    gap = np.minimum(np.abs(adjusted - lo), np.abs(adjusted - hi))
    assert ((adjusted < lo) | (adjusted > hi)).all()
    assert float(gap.min()) > 100.0 * tol
    # The exempt best-holder is penalised under the bound, not restarted.
    for i, role in enumerate(case.roles):
      if role == 'best':
        row = case.start + i
        assert o64.perts[row] < lb and o64.rewards[row] == case.best
    if case_id == 'base-newbest':
      assert o64.best == np.float32(hi) > case.best
    else:
      assert o64.best == case.best


@pytest.mark.parametrize('name', sw.TR_CASES)
def test_trust_region_variant_has_both_sides(name):
  case = sw.sweep_case(name, 'tr')
  assert float(case.perts[[case.start + i for i in case.near]].max()) <= 0.01
  observed = _observed(case)
  o = sw.oracle_iteration(case, 'ucb', sc.COEF, sw.BEST_VALUE, sc.TR_RADIUS,
                          observed)
  improved = np.array([k == 'improved' for k in o.kinds])
  near = (o.dist.numpy() <= sc.TR_NEAR) & improved
  far = (o.dist.numpy() >= sc.TR_FAR) & improved
  assert near.sum() >= 2 and far.sum() >= 2, (near.sum(), far.sum())
  assert set(case.near) <= set(np.nonzero(near)[0].tolist())
  assert not bool(o.penalised[torch.from_numpy(near)].any())
  assert bool(o.penalised[torch.from_numpy(far)].all())
  # Nobody within rounding of the radius.
  assert float((o.dist - sc.TR_RADIUS).abs().min()) > 1e-3
  for radius in (0.0, 0.6):
    assert not bool(sw.oracle_iteration(
        case, 'ucb', sc.COEF, sw.BEST_VALUE, radius,
        observed).penalised.any())


@pytest.mark.parametrize('shape', [(25, 200, 10), (9, 64, 3)])
def test_oracle_iteration_reproduces_the_scorer_reference(shape):
  """The glue: on a scorer_cases case, with its xq as the candidates,
  oracle_iteration gives scorer_cases.reference."""
  b, n, d = shape
  scorer = sc.dense_case(b, n, d)
  case = sw.make_sweep_case(2 * b, b, d, n, seed=5)
  case.x, case.ls, case.alpha, case.M = (scorer.x, scorer.ls, scorer.alpha,
                                         scorer.M)
  observed = types.SimpleNamespace(out_cont=scorer.xq.numpy())
  ref = sc.dense_reference(b, n, d)
  for code, acq in enumerate(sc.ACQ_NAMES):
    o = sw.oracle_iteration(case, acq, sc.COEF, sw.BEST_VALUE, 0.0, observed)
    assert torch.equal(o.k, ref.k) and torch.equal(o.mean, ref.mean)
    assert torch.equal(o.quad, ref.quad) and torch.equal(o.sd, ref.sd)
    assert torch.equal(o.dist, ref.dist)
    assert torch.equal(o.score, sc.acquisition(code, ref.mean, ref.sd,
                                               sc.COEF, sw.BEST_VALUE))
  # The fp32 distance differs from it by the rounding of one subtraction.
  d32 = sw.dist_f32(scorer.xq.numpy(), scorer.x.numpy())
  assert float(np.abs(d32 - ref.dist.numpy()).max()) <= 2.0 ** -24


def test_update_seed_and_iteration_conventions():
  case = sw.sweep_case('base')
  assert (case.n_batches, case.it_start, case.start) == (2, 5, 25)
  assert case.full_iterations() == 5 and case.tiles == 1
  assert sw.sweep_case('B2-stride').tiles == 324 > 256
  assert sw.sweep_case('B-stride').tiles == 100 > 64
  assert sw.sweep_case('large-n').tiles == 4225
  pool, _, dc, _ = sw.CASES['stage-64']
  assert pool * dc == 8192 and pool * sw.CASES['stage-65'][2] == 8320
