"""Times the acquisition sweep of the surrogates that combine several Matern
GPs, with group_scorer='torch' and 'hip' (GP-Bandit, single objective).

Seeded 20-D problem, N = 1000, default budget. Configurations: ensemble_size 3
and 5, and one and two prior studies of N = 1000 each (set_priors). Posteriors
are installed at fixed hyperparameters through gp_model._build_posterior_cache,
so no fit is timed. The two scorers alternate in the same process after a
warm-up sweep each; every timing ends with a device synchronise. Prints one
JSON line per configuration. For the ensembles it also times the bare
group_scores op with the members on one shared x (one x-run: X is read once)
and on G copies of it (G runs: G passes). For the per-kernel split run this
file under `rocprofv3 --kernel-trace --stats -- python tools_group_bench.py`.
"""

import argparse
import json
import time

import numpy as np
import torch

from vizier_amd import pyvizier as vz
from vizier_amd._src.algorithms.core import abstractions as ab
from vizier_amd._src.algorithms.designers import gp_bandit
from vizier_amd._src.algorithms.optimizers import eagle, vectorized
from vizier_amd._src.gp import gp_model
from vizier_amd._src.ops import dispatch

CONFIGS = [('ensemble3', 3, 0), ('ensemble5', 5, 0), ('prior1', 1, 1),
           ('prior2', 1, 2)]


def _fixed_train_gp(x, y, *, seed=0, ensemble_size=1, **_):
  """train_gp's result at seeded hyperparameters: amp 1, noise 1e-3, mean 0,
  lengthscales (0.5 + U) sqrt(d / 4), one draw per member."""
  d = x.shape[1]
  g = torch.Generator().manual_seed(seed)
  members = []
  for _ in range(max(ensemble_size, 1)):
    ls = (0.5 + torch.rand(d, generator=g)) * (d / 4) ** 0.5
    values = [(0.0, gp_model._LOG_AMP_BOUNDS),
              (float(np.log(1e-3)), gp_model._LOG_NOISE_BOUNDS),
              (0.0, gp_model._MEAN_BOUNDS)]
    values += [(float(v), gp_model._LOG_LS_BOUNDS) for v in ls.log()]
    raw = torch.tensor([gp_model._from_bounded(v, *b) for v, b in values])
    members.append(gp_model._build_posterior_cache(
        x, y.reshape(-1), raw.to(x), 0.0, precompute_inverse=True))
  return members[0] if len(members) == 1 else \
      gp_model.EnsembleGPPosterior(members=members)


def _trials(rng, n, d, shift):
  trials = []
  for uid, v in enumerate(rng.uniform(size=(n, d)), 1):
    trials.append(vz.Trial({f'x{i}': float(v[i]) for i in range(d)}, id=uid))
    trials[-1].complete(vz.Measurement(
        metrics={'obj': float(-((v - 0.3 - shift) ** 2).sum())}))
  return trials


def _designer(scorer, n, d, ensemble, priors, evaluations):
  rng = np.random.default_rng(0)
  problem = vz.ProblemStatement()
  for i in range(d):
    problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
  problem.metric_information.append(vz.MetricInformation(
      name='obj', goal=vz.ObjectiveMetricGoal.MAXIMIZE))
  des = gp_bandit.VizierGPBandit(problem, gp_bandit.GPBanditConfig(
      ensemble_size=ensemble, group_scorer=scorer,
      max_evaluations=evaluations, device='cuda'), seed=1)
  if priors:
    des.set_priors([ab.CompletedTrials(_trials(rng, n, d, 0.1 * (p + 1)))
                    for p in range(priors)])
  des.update(ab.CompletedTrials(_trials(rng, n, d, 0.0)), ab.ActiveTrials())
  des._fit()
  return des, des._score_factory(1)[0]


def _sweep(des, score_fn, evaluations):
  optimizer = vectorized.VectorizedOptimizerFactory(
      eagle_config=eagle.EagleStrategyConfig(), max_evaluations=evaluations,
      suggestion_batch_size=25)(
          n_continuous=des._codec.n_continuous,
          categorical_sizes=des._codec.categorical_sizes, seed=3,
          device=des._device, dtype=torch.float32)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  optimizer.optimize(score_fn, count=1)
  torch.cuda.synchronize()
  return time.perf_counter() - t0, optimizer.last_used_graph


def _op_us(des, cloned, calls=300):
  """Microseconds per bare group_scores call on 25 candidates."""
  from vizier_amd._src.gp import acquisitions as acq_lib
  posts = des._posteriors[0].members
  share = [1.0 / len(posts)] * len(posts)
  ops_ = list(acq_lib.GroupScoringFunction(
      posts, share, share, 1.0, acq_lib.UCB(1.8),
      des._make_trust_region()).operands())
  if cloned:
    ops_[0] = [x.clone() for x in ops_[0]]
  xs = torch.rand(25, posts[0].x.shape[1], device='cuda')
  ext = dispatch.require_ext()
  for timed in (False, True):   # the first pass warms up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
      ext.group_scores(xs, *ops_, 0, 1.8, 0.0, 0.3)
    torch.cuda.synchronize()
  return 1e6 * (time.perf_counter() - t0) / calls


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int, default=1000)
  ap.add_argument('--d', type=int, default=20)
  ap.add_argument('--evaluations', type=int, default=75000)
  ap.add_argument('--repeats', type=int, default=3)
  args = ap.parse_args()
  gp_model.train_gp = _fixed_train_gp
  for name, ensemble, priors in CONFIGS:
    runs = {s: _designer(s, args.n, args.d, ensemble, priors,
                         args.evaluations) for s in ('torch', 'hip')}
    times, graph = {s: [] for s in runs}, {}
    for rep in range(args.repeats + 1):   # repeat 0 is the warm-up
      for s, (des, fn) in runs.items():
        dt, graph[s] = _sweep(des, fn, args.evaluations)
        if rep:
          times[s].append(dt)
    out = {'config': name, 'n': args.n, 'd': args.d,
           'evaluations': args.evaluations,
           'sweep_s_torch': sorted(times['torch']),
           'sweep_s_hip': sorted(times['hip']), 'used_graph': graph}
    if ensemble > 1:
      out['op_us_shared_x'] = _op_us(runs['hip'][0], cloned=False)
      out['op_us_cloned_x'] = _op_us(runs['hip'][0], cloned=True)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
  main()
