"""CPU self-check of tests/designer_cases.py (no GPU needed).

Proves that the cases can see what tests/test_designer_scorers.py is there
to catch: candidates sit on both sides of the trust radius and clear of it,
the excluded columns matter, the PE penalty is active on some candidates
and not on others, a swapped posterior or the wrong variance posterior moves
the oracle by more than 100x the tolerance (one named exception: SWAP_FLOOR), and the designers' own closures,
run in fp32 torch on the CPU, agree with the fp64 oracle within the bounds.
"""

import pytest
import torch

import designer_cases as dc

CPU = 'cpu'
UCBPE_IDS = [r[0] for r in dc.UCBPE_ROWS]
PE_IDS = [r[0] for r in dc.UCBPE_ROWS if not r[4]]
MO_IDS = [r[0] for r in dc.UCBPE_ROWS if r[2] == 2]
PENDING_PE_IDS = [r[0] for r in dc.UCBPE_ROWS if not r[4] and r[3] == 2]


@pytest.mark.parametrize('space', ['float', 'mixed'])
def test_mask_dof_and_radius_match_the_converter(space):
  from vizier_amd._src.gp import acquisitions as acq_lib
  setup = dc.ucbpe_setup(space, 1, 2, CPU)
  mask, n_cat = acq_lib.converter_trust_masks(setup.designer._converter)
  assert [int(v) for v in mask] == dc.MASKS[space]
  assert sum(1 for v in mask if not v) + n_cat == dc.DOF
  if space == 'mixed':
    # Excluded columns 1 and 3..5: not one contiguous run.
    assert dc.MASKS[space] == [0, 1, 0, 1, 1, 1, 0]
  for rows in (setup.x_all[:dc.N_DONE], setup.x_all):
    region = acq_lib.TrustRegion.for_converter(rows, setup.designer._converter)
    assert region.trust_radius == pytest.approx(dc.radius(rows.shape[0]),
                                                abs=1e-12)
  assert 0.3 < dc.radius(12) < dc.radius(14) < 0.4


@pytest.mark.parametrize('row', UCBPE_IDS)
def test_candidates_straddle_the_radius(row):
  setup, cands, use_ucb = dc.ucbpe_case(row, True, CPU)
  d = setup.designer
  assert setup.x_all.shape[0] == dc.N_DONE + setup.n_pending
  assert d._posterior.x.shape[0] == dc.N_DONE
  if setup.n_pending == 0:
    assert setup.x_all is d._posterior.x
  # The hand-built dense rows are what the codec decodes the batch to.
  decoded = d._codec.decode(cands.batch(CPU))[:, 0, :]
  assert torch.equal(decoded, cands.dense)
  assert cands.dense.shape[0] == dc.B
  s = dc.ucbpe_oracle(setup, cands, use_ucb)
  r = s.radius
  assert r == dc.radius(setup.x_all.shape[0]) and r < 0.5
  assert int(s.penalised.sum()) >= dc.B // 4
  assert int((~s.penalised).sum()) >= dc.B // 4
  assert float((s.dist - r).abs().min()) >= 0.02
  assert float(s.dist[~s.penalised].max()) <= dc.NEAR
  assert float(s.dist[s.penalised].min()) >= r + 0.05
  assert bool((s.value[s.penalised] < -1e4).all())
  assert bool((s.value[~s.penalised].abs() < 100.0).all())
  if setup.space == 'mixed':
    # With no column excluded every near candidate but the `close` ones
    # would be outside as well, through k alone, the category alone or both.
    plain = dc.min_linf(cands.dense.double(), setup.x_all.double(),
                        [0] * cands.dense.shape[1])
    moved = ~s.penalised & ~cands.close
    assert int(moved.sum()) >= 8
    assert float(plain[moved].min()) > r + 0.05
    for cols in ([0, 0, 0, 1, 1, 1, 0], [0, 1, 0, 0, 0, 0, 0]):
      part = dc.min_linf(cands.dense.double(), setup.x_all.double(), cols)
      assert int((part[moved] > r + 0.05).sum()) >= 3
  # sd is not at the clamp anywhere a value is compared.
  for key in ('sd', 'sd_all'):
    if key in s.info:
      assert float(s.info[key][~s.penalised].min()) >= 0.1 * dc.AMP, key
  # Sanity only: the bounds are small against scores of order 1.
  assert float(s.tol[~s.penalised].max()) < 0.3
  assert float(s.tol.min()) > 0.0


@pytest.mark.parametrize('row', PE_IDS)
def test_pe_penalty_is_active_on_some_candidates_only(row):
  setup, cands, _ = dc.ucbpe_case(row, True, CPU)
  s = dc.ucbpe_oracle(setup, cands, False)
  gap = s.info['gap'][~s.penalised]
  assert bool((gap < 0).any()) and bool((gap > 0).any())
  # The threshold's observed point is a clear winner: its UCB lead is above
  # twice the error an fp32 evaluation of an observed UCB can have, so the
  # argmax cannot flip.
  assert s.info['obs_ucb_gap'] > 2.5 * s.info['obs_ucb_tol']
  # Without the trust region every candidate is compared by value.
  setup_off, cands_off, _ = dc.ucbpe_case(row, False, CPU)
  off = dc.ucbpe_oracle(setup_off, cands_off, False)
  assert not bool(off.penalised.any()) and off.dist is None
  assert bool((off.info['gap'] < 0).any() and (off.info['gap'] > 0).any())


@pytest.mark.parametrize('row', UCBPE_IDS)
def test_sd_clears_the_floor_with_the_region_off(row):
  # All 32 candidates are compared by value on this leg.
  setup, cands, use_ucb = dc.ucbpe_case(row, False, CPU)
  off = dc.ucbpe_oracle(setup, cands, use_ucb)
  assert not bool(off.penalised.any()) and off.dist is None
  keys = [key for key in ('sd', 'sd_all') if key in off.info]
  assert keys == (['sd'] if use_ucb else ['sd', 'sd_all'])
  for key in keys:
    assert float(off.info[key].min()) >= 0.1 * dc.AMP, key


def _moved(right, wrong):
  """Largest |wrong - right| / tolerance over the candidates compared by
  value."""
  keep = ~right.penalised
  return float(((wrong.value - right.value).abs() / right.tol)[keep].max())


# Largest |swapped - right| / bound that a row must exceed, (region on,
# region off). More than 100 on both legs everywhere but mo-ucb-float with
# the region ON, the named exception: it measures 5.5 there and 260 with the
# region off. In the float space no column is excluded, so every candidate
# compared by value with the region on lies within 0.05 of the data in EVERY
# column; sd is about 0.1 amp there, and the bound, which carries
# sum |k||K^-1||k| / (2 sd), is at its loosest (2e-2 .. 1e-1).
SWAP_FLOOR = {'mo-ucb-float': (4.0, 100.0)}


def _swap_moved(case, oracle):
  moved = []
  for trust_region in (True, False):
    args = case(trust_region)
    moved.append(_moved(oracle(*args), oracle(*args, swap_metrics=True)))
  return moved


@pytest.mark.parametrize('row', MO_IDS)
def test_swapped_metric_posteriors_move_the_oracle(row):
  moved = _swap_moved(lambda tr: dc.ucbpe_case(row, tr, CPU), dc.ucbpe_oracle)
  floor = SWAP_FLOOR.get(row, (100.0, 100.0))
  print(f'OBSERVED swap {row}: region on {moved[0]:.1f}, off {moved[1]:.1f}')
  assert moved[0] > floor[0] and moved[1] > floor[1], moved


def test_swapped_bandit_posteriors_move_the_oracle():
  moved = _swap_moved(lambda tr: dc.bandit_case('fp32', tr, CPU),
                      dc.bandit_oracle)
  assert moved[0] > 100.0 and moved[1] > 100.0, moved


@pytest.mark.parametrize('row', PENDING_PE_IDS)
def test_posterior_in_place_of_var_post_moves_the_oracle(row):
  setup, cands, _ = dc.ucbpe_case(row, True, CPU)
  d = setup.designer
  var_post = d._variance_posterior(setup.x_all)
  assert var_post.x.shape[0] == 14 and d._posterior.x.shape[0] == 12
  assert setup.n_pending == 2
  assert var_post.x is setup.x_all
  moved = _moved(
      dc.ucbpe_oracle(setup, cands, False),
      dc.ucbpe_oracle(setup, cands, False, posterior_as_var_post=True))
  assert moved > 100.0, moved


@pytest.mark.parametrize('trust_region', [True, False], ids=['tr', 'no-tr'])
@pytest.mark.parametrize('row', UCBPE_IDS)
def test_cpu_closure_agrees_with_the_oracle(row, trust_region):
  """The designer's own closure (fp32 torch on the CPU: the eager paths)
  against the fp64 oracle, within the bounds the GPU test uses."""
  setup, cands, use_ucb = dc.ucbpe_case(row, trust_region, CPU)
  want = dc.ucbpe_oracle(setup, cands, use_ucb)
  score_fn = setup.designer._one_score_fn(use_ucb, setup.x_all)
  got = score_fn(cands.batch(CPU)).double()
  ratio = (got - want.value).abs() / want.tol
  print(f'OBSERVED cpu {row} tr={trust_region}: {float(ratio.max()):.3f} '
        f'of the bound')
  assert float(ratio.max()) <= 1.0


@pytest.mark.parametrize('trust_region', [True, False], ids=['tr', 'no-tr'])
def test_cpu_bandit_closure_agrees_with_the_oracle(trust_region):
  setup, cands = dc.bandit_case('fp32', trust_region, CPU)
  want = dc.bandit_oracle(setup, cands)
  score_fn, n_parallel = setup.designer._score_factory(1)
  assert n_parallel == 1
  got = score_fn(cands.batch(CPU)).double()
  ratio = (got - want.value).abs() / want.tol
  print(f'OBSERVED cpu bandit tr={trust_region}: {float(ratio.max()):.3f} '
        f'of the bound')
  assert float(ratio.max()) <= 1.0
