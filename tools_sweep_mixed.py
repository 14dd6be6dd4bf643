"""One `optimize` call of the reference budget on a mixed search space.

75,000 evaluations, batch 25, pool 100, N = 1000 completed trials; 12
continuous and 8 categorical parameters with 2 to 6 values (D = 44 dense
columns). Prints the path the optimizer took, the wall time of the second
(warm) call and, on the megakernel path, the per-phase ticks of workgroup 0
(eagle_sweep_mixed.hip). Run it in a fresh process per measurement;
VIZIER_AMD_MEGAKERNEL_MIXED=0 gives the hipGraph path.
"""
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
from vizier_amd._src.algorithms.optimizers.eagle import (  # noqa: E402
    EagleStrategyConfig,
)
from vizier_amd._src.algorithms.optimizers.vectorized import (  # noqa: E402
    VectorizedOptimizerFactory,
)

CAT_SIZES = [2, 3, 4, 5, 6, 2, 3, 4]
N_CONT, N_TRIALS, EVALS, BATCH = 12, 1000, 75000, 25

problem = vz.ProblemStatement()
root = problem.search_space.root
for i in range(N_CONT):
  root.add_float_param(f'x{i}', -5.0, 5.0)
for j, size in enumerate(CAT_SIZES):
  root.add_categorical_param(f'c{j}', [f'v{k}' for k in range(size)])
problem.metric_information.append(vz.MetricInformation(
    name='obj', goal=vz.ObjectiveMetricGoal.MAXIMIZE))

rng = np.random.default_rng(0)
trials = []
for uid in range(1, N_TRIALS + 1):
  xs = rng.uniform(-5, 5, N_CONT)
  cs = [int(rng.integers(0, s)) for s in CAT_SIZES]
  params = {f'x{i}': float(v) for i, v in enumerate(xs)}
  params.update({f'c{j}': f'v{c}' for j, c in enumerate(cs)})
  t = vz.Trial(params, id=uid)
  t.complete(vz.Measurement(metrics={
      'obj': float(-(xs ** 2).sum() / N_CONT + sum(c == 0 for c in cs))}))
  trials.append(t)

designer = VizierGPBandit(problem, GPBanditConfig(
    max_evaluations=EVALS, suggestion_batch_size=BATCH, device='cuda'),
    seed=0)
designer.update(CompletedTrials(trials), ActiveTrials())
designer.suggest(1)
score_fn, _ = designer._score_factory(1)
fac = VectorizedOptimizerFactory(
    eagle_config=EagleStrategyConfig(pool_size=100), max_evaluations=EVALS,
    suggestion_batch_size=BATCH)
opt = fac(n_continuous=N_CONT, categorical_sizes=CAT_SIZES, seed=0,
          device='cuda')
opt.optimize(score_fn, count=1)  # warm
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
    'megakernel': bool(opt.last_used_megakernel),
    'graph': bool(opt.last_used_graph), 'error': opt.last_graph_error,
    'pool': strat.pool_size, 'wall_ms': round(wall * 1e3, 2),
    'us_per_iter': round(wall / (EVALS // BATCH) * 1e6, 2),
    'best_reward': float(result.rewards[0]),
}
if opt.last_used_megakernel:
  # 100 MHz ticks per iteration; barrier columns include workgroup 0's
  # wait for the slowest workgroup. A.cat is the categorical mutation
  # inside A (pair pass, its barrier, per-parameter scan).
  names = ['A', 'barA', 'B', 'barB', 'B2', 'barB2', 'RC', 'barC',
           'B.stage', 'B.main', 'A.cat']
  out['ticks_per_iter'] = {
      nm: round(c / iters) for nm, c in zip(names, delta)}
print(json.dumps(out))
