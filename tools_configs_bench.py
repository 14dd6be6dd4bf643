"""Measures BASELINE.json's milestone configs 2-5 on ONE MI355X.

  2: GP-UCB 8D, N=500, bf16 candidate grams
  3: GP-EI (qEI) 20D, N=2000, suggest count=8
  4: GP-Bandit 50D, N=10000, 1.25M-candidate sweep (the per-GPU slice
     of the 10M-candidate DP=8 config; the driver runs the multi-GPU
     scaling itself)
  5: Multi-objective HV-scalarized UCB + trust region, 30D, fp8 grams

  setpe: GP-UCB-PE set-PE batch, 20D, N=1000, suggest count=8 with
     optimize_set_acquisition_for_exploration (only when asked for by name)

Each reports suggest() wall-clock (mean over a few calls, first call
excluded: it pays hipGraph/megakernel warmup).

Usage: tools_configs_bench.py [2|3|4|5|setpe] [--qei-scorer {torch,hip}]
                              [--set-pe-scorer {torch,hip}]
--qei-scorer selects config 3's qEI set scorer and --set-pe-scorer the
set-PE scorer of config setpe (default torch, so recorded numbers stay
comparable); these two configs also print every repetition, the sweep-only
time (fit cached) and whether the sweep ran as a hipGraph.
"""

import json
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from vizier_amd import pyvizier as vz
from vizier_amd._src.algorithms.core.abstractions import (
    ActiveTrials,
    CompletedTrials,
)
from vizier_amd._src.algorithms.designers.gp_bandit import (
    GPBanditConfig,
    VizierGPBandit,
)


def make_problem(dim, metrics=('obj',)):
  p = vz.ProblemStatement()
  for i in range(dim):
    p.search_space.root.add_float_param(f'x{i}', -5.0, 5.0)
  p.metric_information = vz.MetricsConfig([
      vz.MetricInformation(name=m, goal=vz.ObjectiveMetricGoal.MAXIMIZE)
      for m in metrics])
  return p


def preload(designer, dim, n_trials, metrics=('obj',), seed=0):
  rng = np.random.default_rng(seed)
  trials = []
  for uid in range(1, n_trials + 1):
    x = rng.uniform(-5, 5, dim)
    t = vz.Trial({f'x{i}': float(x[i]) for i in range(dim)}, id=uid)
    vals = {m: float(-((x - k) ** 2).sum() / dim)
            for k, m in enumerate(metrics)}
    t.complete(vz.Measurement(metrics=vals))
    trials.append(t)
  designer.update(CompletedTrials(trials), ActiveTrials())


def timed_suggest(designer, count=1, reps=3, times=None):
  designer.suggest(count)  # warmup (fit + graph capture)
  torch.cuda.synchronize()
  times = [] if times is None else times
  uid = 10_000_000
  for _ in range(reps):
    t0 = time.perf_counter()
    sugg = designer.suggest(count)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
    # Complete one so the fit isn't trivially cached.
    uid += 1
    t = sugg[0].to_trial(uid)
    t.complete(vz.Measurement(metrics={
        m.name: 0.0 for m in designer._problem.metric_information}))
    designer.update(CompletedTrials([t]), ActiveTrials())
  return float(np.mean(times) * 1e3)


def run_one(which: str) -> None:
  main(only=which)


def main(only=None, qei_scorer='torch', set_pe_scorer='torch'):
  out = {}

  # Config 2: 8D, N=500, bf16 grams.
  for dtype in (('fp32', 'bf16') if only in (None, '2') else ()):
    d = VizierGPBandit(make_problem(8), GPBanditConfig(
        max_evaluations=75000, device='cuda',
        scorer_gram_dtype=dtype), seed=0)
    preload(d, 8, 500)
    ms = timed_suggest(d)
    out[f'config2_8d_n500_{dtype}'] = ms
    print(f'config 2 (8D N=500, {dtype}): {ms:.1f} ms/suggest',
          flush=True)

  # Config 3: 20D, N=2000, qEI count=8.
  if only in (None, '3'):
    _config3(out, qei_scorer)

  # Config 4: 50D, N=10000, 1.25M evals (per-GPU slice of 10M DP=8).
  if only in (None, '4'):
    _config4(out)

  # Config 5: 30D MO + trust region, fp8 grams.
  if only in (None, '5'):
    _config5(out)

  if only == 'setpe':
    _config_setpe(out, set_pe_scorer)

  print(json.dumps(out))
  import os
  path = 'gpurun_out/configs_bench.json'
  old = json.load(open(path)) if os.path.exists(path) else {}
  old.update(out)
  with open(path, 'w') as f:
    json.dump(old, f, indent=2)


def _config3(out, qei_scorer='torch'):
  d = VizierGPBandit(make_problem(20), GPBanditConfig(
      max_evaluations=75000, acquisition='qei', qei_scorer=qei_scorer,
      device='cuda'), seed=0)
  preload(d, 20, 2000)
  times = []
  ms = timed_suggest(d, count=8, reps=5, times=times)
  # The default scorer keeps the historical key.
  key = 'config3_20d_n2000_qei8' + ('' if qei_scorer == 'torch'
                                    else f'_{qei_scorer}')
  out[key] = ms
  print(f'config 3 (20D N=2000 qEI q=8, {qei_scorer} scorer): {ms:.1f} '
        'ms/suggest(8); reps ' + ' '.join(f'{t * 1e3:.1f}' for t in times),
        flush=True)
  # Sweep alone: the fit is cached after the first call.
  d._fit()
  sweeps = []
  for _ in range(5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d._gp_suggestions(8)
    torch.cuda.synchronize()
    sweeps.append((time.perf_counter() - t0) * 1e3)
  opt = d._last_optimizer
  out[key + '_sweep_ms'] = float(np.median(sweeps))
  out[key + '_used_graph'] = bool(opt.last_used_graph)
  print(f'config 3 sweep only: median {np.median(sweeps):.1f} ms, min '
        f'{min(sweeps):.1f}, max {max(sweeps):.1f}; hipGraph path: '
        f'{opt.last_used_graph} (graph error: {opt.last_graph_error})',
        flush=True)


def _config_setpe(out, set_pe_scorer='torch'):
  from vizier_amd._src.algorithms.designers.gp_ucb_pe import (
      UCBPEConfig,
      VizierGPUCBPEBandit,
  )
  d = VizierGPUCBPEBandit(make_problem(20), UCBPEConfig(
      max_evaluations=75000, optimize_set_acquisition_for_exploration=True,
      set_pe_scorer=set_pe_scorer, device='cuda'), seed=0)
  preload(d, 20, 1000)
  times = []
  ms = timed_suggest(d, count=8, reps=3, times=times)
  key = f'setpe_20d_n1000_q8_{set_pe_scorer}'
  out[key] = ms
  print(f'config setpe (20D N=1000 suggest(8), {set_pe_scorer} scorer): '
        f'{ms:.1f} ms/suggest(8); reps '
        + ' '.join(f'{t * 1e3:.1f}' for t in times), flush=True)
  # The set phase alone (variance posterior + the 7-member set sweep): the
  # fit is cached after the first call.
  d._fit()
  sweeps = []
  for _ in range(5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    d._optimize_set(d._posterior.x, 7)
    torch.cuda.synchronize()
    sweeps.append((time.perf_counter() - t0) * 1e3)
  opt = d._last_set_optimizer
  out[key + '_sweep_ms'] = float(np.median(sweeps))
  out[key + '_used_graph'] = bool(opt.last_used_graph)
  print(f'config setpe set sweep only: median {np.median(sweeps):.1f} ms, '
        f'min {min(sweeps):.1f}, max {max(sweeps):.1f}; hipGraph path: '
        f'{opt.last_used_graph} (graph error: {opt.last_graph_error})',
        flush=True)


def _config4(out):
  d = VizierGPBandit(make_problem(50), GPBanditConfig(
      max_evaluations=1_250_000, device='cuda'), seed=0)
  preload(d, 50, 10000)
  ms = timed_suggest(d, reps=2)
  out['config4_50d_n10000_1p25M'] = ms
  print(f'config 4 (50D N=10000, 1.25M evals): {ms:.1f} ms/suggest',
        flush=True)


def _config5(out):
  for dtype in ('fp32', 'fp8'):
    d = VizierGPBandit(make_problem(30, metrics=('f1', 'f2')),
                       GPBanditConfig(max_evaluations=75000,
                                      device='cuda',
                                      scorer_gram_dtype=dtype), seed=0)
    preload(d, 30, 1000, metrics=('f1', 'f2'))
    ms = timed_suggest(d)
    out[f'config5_30d_mo_{dtype}'] = ms
    print(f'config 5 (30D MO N=1000, {dtype}): {ms:.1f} ms/suggest',
          flush=True)
    del d
    torch.cuda.empty_cache()


if __name__ == '__main__':
  import argparse
  parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
  parser.add_argument('only', nargs='?',
                      choices=['2', '3', '4', '5', 'setpe'],
                      help='run this config alone (default: 2-5)')
  parser.add_argument('--qei-scorer', choices=['torch', 'hip'],
                      default='torch', help="config 3's qEI set scorer")
  parser.add_argument('--set-pe-scorer', choices=['torch', 'hip'],
                      default='torch', help="config setpe's set-PE scorer")
  args = parser.parse_args()
  main(only=args.only, qei_scorer=args.qei_scorer,
       set_pe_scorer=args.set_pe_scorer)
