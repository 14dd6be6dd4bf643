"""One multi-objective sweep of the reference budget, timed.

75,000 evaluations, batch 25, N = 1000 completed trials, `--dim` continuous
parameters (20 or 30) and `--metrics` objectives (2 or 3), the designer's
defaults otherwise (pool 50 at 20D, 75 at 30D; 1000 scalarisations). Prints
the path the optimizer took, the wall time of a warm `optimize` call as us
per iteration, the wall time of a warm `suggest(1)` and, on the megakernel
path, the per-phase ticks of workgroup 0 (eagle_sweep_mo.hip). Run it in a
fresh process per measurement; VIZIER_AMD_MEGAKERNEL_MO=0 gives the hipGraph
path.
"""
import argparse
import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from vizier_amd import pyvizier as vz  # noqa: E402
from vizier_amd._src.algorithms.core.abstractions import (  # noqa: E402
    ActiveTrials,
    CompletedTrials,
)
from vizier_amd._src.algorithms.designers.gp_bandit import (  # noqa: E402
    GPBanditConfig,
    VizierGPBandit,
)

p = argparse.ArgumentParser()
p.add_argument('--dim', type=int, default=20)
p.add_argument('--metrics', type=int, default=2)
p.add_argument('--trials', type=int, default=1000)
args = p.parse_args()
EVALS, BATCH = 75000, 25

problem = vz.ProblemStatement()
for i in range(args.dim):
  problem.search_space.root.add_float_param(f'x{i}', -5.0, 5.0)
names = [f'f{m}' for m in range(args.metrics)]
problem.metric_information = vz.MetricsConfig([
    vz.MetricInformation(name=n, goal=vz.ObjectiveMetricGoal.MAXIMIZE)
    for n in names])

rng = np.random.default_rng(0)
centres = rng.uniform(-3, 3, (args.metrics, args.dim))
trials = []
for uid in range(1, args.trials + 1):
  xs = rng.uniform(-5, 5, args.dim)
  t = vz.Trial({f'x{i}': float(v) for i, v in enumerate(xs)}, id=uid)
  t.complete(vz.Measurement(metrics={
      n: float(-((xs - c) ** 2).sum() / args.dim)
      for n, c in zip(names, centres)}))
  trials.append(t)

# The fit is not what is measured: one restart, few iterations.
designer = VizierGPBandit(problem, GPBanditConfig(
    max_evaluations=EVALS, suggestion_batch_size=BATCH, ard_restarts=1,
    ard_max_iters=10, device='cuda'), seed=0)
designer.update(CompletedTrials(trials), ActiveTrials())
designer.suggest(1)  # fit + warm
torch.cuda.synchronize()
t0 = time.perf_counter()
designer.suggest(1)
torch.cuda.synchronize()
suggest_ms = (time.perf_counter() - t0) * 1e3

opt = designer._last_optimizer
score_fn, _ = designer._score_factory(1)
strat = opt.strategy
base = strat._iter_t[2:].clone()
torch.cuda.synchronize()
t0 = time.perf_counter()
result = opt.optimize(score_fn, count=1)
torch.cuda.synchronize()
wall = time.perf_counter() - t0
delta = (strat._iter_t[2:] - base).cpu().numpy().astype(float)
iters = EVALS // BATCH - (strat.pool_size // strat.batch_size + 2)
out = {
    'dim': args.dim, 'metrics': args.metrics, 'n': args.trials,
    'megakernel': bool(opt.last_used_megakernel),
    'graph': bool(opt.last_used_graph), 'error': opt.last_graph_error,
    'pool': strat.pool_size, 'sweep_ms': round(wall * 1e3, 2),
    'us_per_iter': round(wall / (EVALS // BATCH) * 1e6, 2),
    'suggest_ms': round(suggest_ms, 2),
    'best_reward': float(result.rewards[0]),
}
if opt.last_used_megakernel:
  # 100 MHz ticks per iteration; the barrier columns include workgroup 0's
  # wait for the slowest workgroup.
  names = ['A', 'barA', 'B', 'barB', '-', '-', 'RC', '-', 'B.stage',
           'B.main']
  out['ticks_per_iter'] = {
      nm: round(c / iters) for nm, c in zip(names, delta) if nm != '-'}
print(json.dumps(out))
