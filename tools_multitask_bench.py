"""Times the acquisition sweep of a separable multitask surrogate with
multitask_scorer='torch' and 'hip' (GP-Bandit, multi-objective branch).

Seeded 20-D problem, N = 1000, M = 2 and 3. One posterior is installed through
multitask.posterior_from_params, so no fit is timed. The two scorers alternate
in the same process after a warm-up sweep each; every timing ends with a device
synchronise. Prints one JSON line per M. For the per-kernel split run this file
under `rocprofv3 --kernel-trace --stats -- python tools_multitask_bench.py`;
mt_quadform_kernel moves M * items * 64 * 64 * 4 bytes of W per call
(items = tiles (tiles + 1) / 2, tiles = ceil(N / 64)).
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
from vizier_amd._src.gp import multitask


def _designer(scorer, n, d, m, evaluations):
  rng = np.random.default_rng(0)

  def fixed(x, y, with_fused_cache=False, **_):
    g = torch.Generator().manual_seed(1)
    chol = torch.tril(torch.rand(m, m, generator=g) - 0.5, -1) + torch.eye(m)
    chol = chol / chol.norm(dim=-1, keepdim=True)
    params = multitask.MultitaskParams(
        noise=torch.tensor(1e-3).to(x), means=torch.zeros(m).to(x),
        lengthscales=(0.5 + torch.rand(d, generator=g)).to(x) * (d / 4) ** 0.5,
        task_chol=chol.to(x))
    return multitask.posterior_from_params(
        x, y, params, with_fused_cache=with_fused_cache)
  multitask.train_multitask_gp = fixed

  problem = vz.ProblemStatement()
  for i in range(d):
    problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
  for t in range(m):
    problem.metric_information.append(vz.MetricInformation(
        name=f'm{t}', goal=vz.ObjectiveMetricGoal.MAXIMIZE))
  des = gp_bandit.VizierGPBandit(problem, gp_bandit.GPBanditConfig(
      multitask_type='separable', multitask_scorer=scorer,
      max_evaluations=evaluations, device='cuda'), seed=1)
  trials = []
  for uid, v in enumerate(rng.uniform(size=(n, d)), 1):
    trials.append(vz.Trial({f'x{i}': float(v[i]) for i in range(d)}, id=uid))
    trials[-1].complete(vz.Measurement(metrics={
        f'm{t}': float(-((v - 0.3 - 0.1 * t) ** 2).sum()) for t in range(m)}))
  des.update(ab.CompletedTrials(trials), ab.ActiveTrials())
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


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int, default=1000)
  ap.add_argument('--d', type=int, default=20)
  ap.add_argument('--evaluations', type=int, default=75000)
  ap.add_argument('--repeats', type=int, default=3)
  args = ap.parse_args()
  for m in (2, 3):
    runs = {s: _designer(s, args.n, args.d, m, args.evaluations)
            for s in ('torch', 'hip')}
    times = {s: [] for s in runs}
    for rep in range(args.repeats + 1):   # repeat 0 is the warm-up
      for s, (des, fn) in runs.items():
        dt, graph = _sweep(des, fn, args.evaluations)
        if rep:
          times[s].append(dt)
    print(json.dumps({
        'n': args.n, 'd': args.d, 'm': m, 'evaluations': args.evaluations,
        'sweep_s_torch': sorted(times['torch']),
        'sweep_s_hip': sorted(times['hip']), 'hip_used_graph': graph}))


if __name__ == '__main__':
  main()
