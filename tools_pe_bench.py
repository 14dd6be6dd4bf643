"""Times GP-UCB-PE's suggest(4) with pe_scorer='torch' and 'hip'.

Seeded 20-D problem, N = 1000, default budget, with 0 and 8 active trials. The
posterior is installed at fixed hyperparameters through
gp_model._build_posterior_cache, so no fit is timed. The two scorers alternate
in the same process after a warm-up suggest each; the designer's random state
is reset before every suggest, so every repeat and both scorers draw the same
UCB / PE member sequence. Every timing ends with a device synchronise. Prints
one JSON line per configuration: the suggest times and, per member, the kind,
the rows of x_all, whether the sweep was captured, the seconds spent building
the scorer (the float64 variance posterior included) and in the sweep. It also
times the bare pe_scores op in PE mode against the two posterior_mean_std
calls it replaces. For the per-kernel split run this file under
`rocprofv3 --kernel-trace --stats -- python tools_pe_bench.py --repeats 1`.
"""

import argparse
import json
import time

import numpy as np
import torch

from vizier_amd import pyvizier as vz
from vizier_amd._src.algorithms.core import abstractions as ab
from vizier_amd._src.algorithms.designers import gp_ucb_pe
from vizier_amd._src.gp import gp_model
from vizier_amd._src.ops import dispatch


def _fixed_train_gp(x, y, **_):
  """train_gp's result at seeded hyperparameters: amp 1, noise 1e-3, mean 0,
  lengthscales (0.5 + U) sqrt(d / 4)."""
  d = x.shape[1]
  ls = (0.5 + torch.rand(d, generator=torch.Generator().manual_seed(0))) * \
      (d / 4) ** 0.5
  values = [(0.0, gp_model._LOG_AMP_BOUNDS),
            (float(np.log(1e-3)), gp_model._LOG_NOISE_BOUNDS),
            (0.0, gp_model._MEAN_BOUNDS)]
  values += [(float(v), gp_model._LOG_LS_BOUNDS) for v in ls.log()]
  raw = torch.tensor([gp_model._from_bounded(v, *b) for v, b in values])
  return gp_model._build_posterior_cache(x, y.reshape(-1), raw.to(x), 0.0,
                                         precompute_inverse=True)


def _designer(scorer, n, d, active, evaluations):
  rng = np.random.default_rng(0)
  problem = vz.ProblemStatement()
  for i in range(d):
    problem.search_space.root.add_float_param(f'x{i}', 0.0, 1.0)
  problem.metric_information.append(vz.MetricInformation(
      name='obj', goal=vz.ObjectiveMetricGoal.MAXIMIZE))
  des = gp_ucb_pe.VizierGPUCBPEBandit(problem, gp_ucb_pe.UCBPEConfig(
      pe_scorer=scorer, max_evaluations=evaluations, device='cuda'), seed=1)
  trials = []
  for uid, v in enumerate(rng.uniform(size=(n + active, d)), 1):
    trials.append(vz.Trial({f'x{i}': float(v[i]) for i in range(d)}, id=uid))
    if uid <= n:
      trials[-1].complete(vz.Measurement(
          metrics={'obj': float(-((v - 0.3) ** 2).sum())}))
  des.update(ab.CompletedTrials(trials[:n]), ab.ActiveTrials(trials[n:]))
  return des


def _timed_suggest(des, count):
  """(seconds, per-member records) of one suggest(count)."""
  members, build = [], []
  one, score = des._optimize_one, des._one_score_fn

  def timed_score(use_ucb, x_all):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = score(use_ucb, x_all)
    torch.cuda.synchronize()
    build.append(time.perf_counter() - t0)
    return out

  def timed_one(use_ucb, x_all):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = one(use_ucb, x_all)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    opt = des._last_optimizer
    members.append({
        'kind': 'ucb' if use_ucb else 'pe', 'rows': int(x_all.shape[0]),
        'path': 'megakernel' if opt.last_used_megakernel else
                'graph' if opt.last_used_graph else 'eager',
        'build_s': round(build[-1], 4), 'sweep_s': round(dt - build[-1], 4)})
    return out

  des._optimize_one, des._one_score_fn = timed_one, timed_score
  des._rng = np.random.default_rng(des._seed)
  des._last_suggest_completed = 0
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  des.suggest(count)
  torch.cuda.synchronize()
  dt = time.perf_counter() - t0
  des._optimize_one, des._one_score_fn = one, score
  return dt, members


def _op_us(des, active, calls=300):
  """Microseconds per PE score of 25 candidates: one pe_scores call, and the
  two posterior_mean_std calls of the 'torch' closure (its elementwise tail
  not included)."""
  from vizier_amd._src.gp import acquisitions as acq_lib
  ext = dispatch.require_ext()
  post = des._posterior
  d = post.x.shape[1]
  x_all = torch.cat([post.x, torch.rand(active, d, device='cuda')]) \
      if active else post.x
  var_post = des._variance_posterior(x_all)
  tr = acq_lib.TrustRegion.for_converter(x_all, des._converter)
  hip = acq_lib.PEScoringFunction(
      post, x_all, var_post, tr, explore_coef=0.5, threshold=0.0,
      penalty_coef=10.0)
  onehot = tr._onehot.to(torch.uint8)
  amp, mean_c = float(post.params.amplitude), float(post.params.mean)
  xs = torch.rand(25, d, device='cuda')

  def two_calls():
    ext.posterior_mean_std(xs, post.x, post.params.lengthscales, amp, mean_c,
                           post.alpha, post.K_inv, onehot)
    ext.posterior_mean_std(xs, x_all, post.params.lengthscales, amp, 0.0,
                           var_post.alpha, var_post.K_inv, onehot)
  out = {}
  for name, fn in (('pe_scores', lambda: hip(xs)),
                   ('two_posterior_mean_std', two_calls)):
    for timed in (False, True):   # the first pass warms up
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(calls):
        fn()
      torch.cuda.synchronize()
    out[name] = round(1e6 * (time.perf_counter() - t0) / calls, 2)
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--n', type=int, default=1000)
  ap.add_argument('--d', type=int, default=20)
  ap.add_argument('--count', type=int, default=4)
  ap.add_argument('--evaluations', type=int, default=75000)
  ap.add_argument('--repeats', type=int, default=3)
  args = ap.parse_args()
  gp_model.train_gp = _fixed_train_gp
  for active in (0, 8):
    runs = {s: _designer(s, args.n, args.d, active, args.evaluations)
            for s in ('torch', 'hip')}
    times, members = {s: [] for s in runs}, {}
    for rep in range(args.repeats + 1):   # repeat 0 is the warm-up
      for s, des in runs.items():
        dt, members[s] = _timed_suggest(des, args.count)
        if rep:
          times[s].append(round(dt, 4))
    print(json.dumps({
        'active': active, 'n': args.n, 'd': args.d, 'count': args.count,
        'evaluations': args.evaluations,
        'suggest_s_torch': sorted(times['torch']),
        'suggest_s_hip': sorted(times['hip']), 'members': members,
        'op_us': _op_us(runs['hip'], active)}), flush=True)


if __name__ == '__main__':
  main()
