"""The fp32 Eagle step kernels (eagle_step.hip) against the NumPy oracle.

ext.eagle_suggest / ext.eagle_update run on every sweep iteration of the
default path, and through the bitwise megakernel-vs-graph test they also
define the sweep megakernel. tests/eagle_f64_oracle.py implements the same
spec with the kernels' RNG bit for bit; here its inputs, config constants
and uniforms are rounded to float32 (what the kernel is handed) and the
formulas are evaluated in float64.

Tolerances come from the reference, never from the kernel:
  continuous   4 x the largest difference between the oracle evaluated in
               NumPy float32 arithmetic and in float64 on the same inputs,
               floored at 8 pool 2^-24 (1 + max|x|), the fp64 test's bound
               at fp32's unit roundoff. The 4 x covers the kernel's other
               summation order and its __expf.
  categorical  equal to the oracle wherever its top-2 `logit + gumbel`
               margin exceeds tau = 4 x the float32-vs-float64 difference
               of `logit + gumbel`; the seeds are chosen so that EVERY
               entry does, which is asserted.
  update       bitwise: one multiply, compares, copies and exact uniforms.
`pytest -rA` prints observed and bound per case as OBSERVED lines.
"""

import dataclasses

import numpy as np
import pytest
import torch

import eagle_f64_oracle as oracle

pytestmark = pytest.mark.gpu

F32 = np.float32

# (pool, batch, dc, cat_sizes, q)
SHAPES = [
    (50, 25, 4, [], 1),
    (100, 25, 20, [], 1),
    (50, 25, 3, [3, 5], 1),
    (128, 32, 0, [3, 3], 1),   # pool at the LDS cap, pure categorical
    (25, 25, 2, [1, 6], 1),    # single batch, a size-1 category
    (50, 25, 3, [3, 5], 3),
    (60, 20, 5, [], 2),
]
# The mutation moves some, not all, categories in these.
SOME_CHANGE = [(50, 25, 3, [3, 5], 1), (50, 25, 3, [3, 5], 3)]


def _id(shape):
  pool, batch, dc, cat_sizes, q = shape
  cats = '+' + ','.join(map(str, cat_sizes)) if cat_sizes else ''
  return f'{pool}x{batch}x{dc}{cats}-q{q}'


@pytest.fixture(scope='module')
def ext():
  from vizier_amd._src.ops import dispatch
  return dispatch.require_ext()  # Fails loudly if the .so is missing.


def config_for(dc):
  """The strategy's defaults; pure-categorical pools take the larger
  categorical perturbation factor (eagle.py::suggest)."""
  from vizier_amd._src.algorithms.optimizers import eagle as eagle_lib
  c = eagle_lib.EagleStrategyConfig()
  return oracle.Config(
      cat_factor=(c.pure_categorical_perturbation_factor if dc == 0
                  else c.categorical_perturbation_factor))


def inputs_f32(pool, q, dc, cat_sizes, seed):
  cont, cat, rewards, perts = oracle.steady_pool(pool, q, dc, cat_sizes,
                                                 seed)
  assert int(np.isinf(rewards).sum()) == 3
  return cont.astype(F32), cat, rewards.astype(F32), perts.astype(F32)


def offset_for(n_batches):
  """Steady state with batch_start > 0 whenever there are two batches."""
  return 3 * n_batches - 1


def suggest_args(cfg):
  return (cfg.visibility, cfg.gravity, cfg.negative_gravity,
          cfg.normalization_scale, cfg.cat_factor, cfg.p_same)


def run_suggest(ext, pool_cont, pool_cat, rewards, perts, cat_sizes, offset,
                n_batches, batch, seed, cfg):
  dev = 'cuda'
  q, dc, dcat = pool_cont.shape[1], pool_cont.shape[2], pool_cat.shape[2]
  iter_t = torch.zeros(12, dtype=torch.long, device=dev)
  iter_t[0] = offset
  iter_t[1] = -7                        # suggest publishes the offset here
  out_cont = torch.empty(batch, q, dc, dtype=torch.float32, device=dev)
  out_cat = torch.empty(batch, q, dcat, dtype=torch.long, device=dev)
  ext.eagle_suggest(
      torch.from_numpy(pool_cont).to(dev), torch.from_numpy(pool_cat).to(dev),
      torch.from_numpy(rewards).to(dev), torch.from_numpy(perts).to(dev),
      torch.tensor(cat_sizes, dtype=torch.long, device=dev), iter_t,
      n_batches, batch, *suggest_args(cfg), seed, out_cont, out_cat,
      max(cat_sizes, default=0))
  assert iter_t[:2].tolist() == [offset, offset]
  return out_cont.cpu().numpy(), out_cat.cpu().numpy()


@pytest.mark.parametrize('shape', SHAPES, ids=[_id(s) for s in SHAPES])
def test_eagle_suggest(ext, shape):
  pool, batch, dc, cat_sizes, q = shape
  cfg = config_for(dc)
  n_batches = pool // batch
  offset, seed = offset_for(n_batches), 2024
  start = (offset % n_batches) * batch
  assert start > 0 or n_batches == 1
  inputs = inputs_f32(pool, q, dc, cat_sizes, seed=pool + dc + q)
  args = (*inputs, cat_sizes, offset, n_batches, batch, seed, cfg)
  want_cont, want_cat, margin, vals64 = oracle.suggest(
      *args, dtype=F32, arith=np.float64, return_vals=True)
  f32_cont, _, _, vals32 = oracle.suggest(
      *args, dtype=F32, arith=F32, return_vals=True)
  got_cont, got_cat = run_suggest(ext, *args)

  if dc:
    floor = 8.0 * pool * 2.0 ** -24 * (1.0 + float(np.abs(inputs[0]).max()))
    tol = max(4.0 * float(np.abs(f32_cont - want_cont).max()), floor)
    err = float(np.abs(got_cont - want_cont).max())
    print(f'OBSERVED suggest {_id(shape)}: continuous {err:.3e} '
          f'(bound {tol:.3e})')
    assert err <= tol
  if cat_sizes:
    tau = 4.0 * float(np.nanmax(np.abs(vals32 - vals64)))
    print(f'OBSERVED suggest {_id(shape)}: smallest top-2 margin '
          f'{margin:.3e} (tau {tau:.3e})')
    assert margin > tau, (margin, tau)
    assert np.array_equal(got_cat, want_cat)
    changed = (want_cat != inputs[1][start:start + batch]).mean()
    if shape in SOME_CHANGE:
      assert 0.0 < changed < 1.0, changed


def update_scenario(pool, batch, dc, cat_sizes, q, n_batches, offset):
  """Even rows improve, odd rows do not; rows 1 and 3 are one penalty away
  from the lower bound (dead), row 4 improves but is already below it
  (dead), and so is row 0, which becomes the new best (exempt)."""
  start = (offset % n_batches) * batch
  rng = np.random.default_rng(8)
  pool_cont, pool_cat, rewards, perts = inputs_f32(pool, q, dc, cat_sizes,
                                                   seed=9)
  rewards[start:start + batch] = rng.normal(size=batch).astype(F32)
  batch_cont = rng.random((batch, q, dc)).astype(F32)
  batch_cat = np.stack([rng.integers(0, s, size=(batch, q))
                        for s in cat_sizes], axis=-1).astype(np.int64)
  delta = np.where(np.arange(batch) % 2 == 0, 0.5, -0.5).astype(F32)
  delta[0] = 5.0
  batch_rewards = rewards[start:start + batch] + delta
  perts[start:start + batch] = 0.16
  perts[start + 1] = perts[start + 3] = 8e-5
  perts[start] = perts[start + 4] = 5e-5
  best = float(rewards[np.isfinite(rewards)].max())
  return (pool_cont, pool_cat, rewards, perts, batch_cont, batch_cat,
          batch_rewards, best)


@pytest.mark.parametrize('q', [1, 3])
def test_eagle_update_bitwise(ext, q):
  cfg = oracle.Config()
  pool, batch, dc, cat_sizes = 50, 25, 3, [3, 5]
  strategy_seed, n_batches, offset = 99, 2, 5
  seed = strategy_seed ^ oracle.UPDATE_SEED_XOR
  start = (offset % n_batches) * batch
  (pool_cont, pool_cat, rewards, perts, batch_cont, batch_cat,
   batch_rewards, best) = update_scenario(pool, batch, dc, cat_sizes, q,
                                          n_batches, offset)
  want = oracle.update(pool_cont, pool_cat, rewards, perts, batch_cont,
                       batch_cat, batch_rewards, cat_sizes, best, offset,
                       n_batches, seed, cfg, dtype=F32)
  kinds = want[5]
  assert {'improved', 'penalised', 'dead'} == set(kinds)
  assert kinds[1] == kinds[3] == kinds[4] == 'dead'
  assert kinds[0] == 'improved' and want[4] == batch_rewards[0] > best

  dev = 'cuda'
  t = [torch.from_numpy(a.copy()).to(dev)
       for a in (pool_cont, pool_cat, rewards, perts)]
  best_t = torch.tensor([best], dtype=torch.float32, device=dev)
  iter_t = torch.zeros(12, dtype=torch.long, device=dev)
  iter_t[0] = -7                        # update reads slot 1, writes slot 0
  iter_t[1] = offset
  ext.eagle_update(
      *t, torch.from_numpy(batch_cont).to(dev),
      torch.from_numpy(batch_cat).to(dev),
      torch.from_numpy(batch_rewards).to(dev),
      torch.tensor(cat_sizes, dtype=torch.long, device=dev), best_t, iter_t,
      n_batches, cfg.penalize_factor, cfg.perturbation_lower_bound,
      cfg.perturbation, seed)
  for name, got, expect in zip(('pool', 'categories', 'rewards', 'perts'),
                               t, want[:4]):
    assert got.cpu().numpy().dtype == expect.dtype
    assert np.array_equal(got.cpu().numpy(), expect), name
  assert float(best_t[0]) == want[4]
  assert iter_t[:2].tolist() == [offset + 1, offset]
  # The refilled rows equal the float32 uniforms exactly, over all q.
  for row in (start + 1, start + 3, start + 4):
    refilled = t[0][row].cpu().numpy().reshape(-1)
    assert np.array_equal(refilled, oracle.uniform(
        seed, offset ^ oracle.TAG_REFILL_CONT,
        row * q * dc + np.arange(q * dc), F32))
  # Rows outside the batch are untouched.
  other = slice(0, start)
  assert np.array_equal(t[0][other].cpu().numpy(), pool_cont[other])
  assert np.array_equal(t[2][other].cpu().numpy(), rewards[other])


# -- argument checks (every one throws before anything is launched) ----------------


class _Call:
  """A valid (50, 25, 3, [3, 5]) call whose operands tests replace."""

  def __init__(self, q=1):
    dev = 'cuda'
    self.cfg = oracle.Config()
    cont, cat, rewards, perts = inputs_f32(50, q, 3, [3, 5], seed=1)
    self.pool_cont = torch.from_numpy(cont).to(dev)
    self.pool_cat = torch.from_numpy(cat).to(dev)
    self.rewards = torch.from_numpy(rewards).to(dev)
    self.perts = torch.from_numpy(perts).to(dev)
    self.cat_sizes = torch.tensor([3, 5], dtype=torch.long, device=dev)
    self.iter_t = torch.full((12,), 5, dtype=torch.long, device=dev)
    self.n_batches, self.batch, self.max_cat = 2, 25, 5
    self.out_cont = torch.empty(25, q, 3, dtype=torch.float32, device=dev)
    self.out_cat = torch.empty(25, q, 2, dtype=torch.long, device=dev)
    self.batch_cont = torch.rand(25, q, 3, device=dev)
    self.batch_cat = torch.zeros(25, q, 2, dtype=torch.long, device=dev)
    self.batch_rewards = torch.zeros(25, device=dev)
    self.best = torch.zeros(1, device=dev)

  def suggest(self, ext, **replace):
    a = dataclasses.replace(_Args(**vars(self)), **replace)
    return ext.eagle_suggest(
        a.pool_cont, a.pool_cat, a.rewards, a.perts, a.cat_sizes, a.iter_t,
        a.n_batches, a.batch, *suggest_args(a.cfg), 1, a.out_cont, a.out_cat,
        a.max_cat)

  def update(self, ext, **replace):
    a = dataclasses.replace(_Args(**vars(self)), **replace)
    return ext.eagle_update(
        a.pool_cont, a.pool_cat, a.rewards, a.perts, a.batch_cont,
        a.batch_cat, a.batch_rewards, a.cat_sizes, a.best, a.iter_t,
        a.n_batches, a.cfg.penalize_factor, a.cfg.perturbation_lower_bound,
        a.cfg.perturbation, 1)


_Args = dataclasses.make_dataclass('_Args', [
    'cfg', 'pool_cont', 'pool_cat', 'rewards', 'perts', 'cat_sizes', 'iter_t',
    'n_batches', 'batch', 'max_cat', 'out_cont', 'out_cat', 'batch_cont',
    'batch_cat', 'batch_rewards', 'best'])


def _big_pool(pool, q=1):
  dev = 'cuda'
  return dict(
      pool_cont=torch.rand(pool, q, 3, device=dev),
      pool_cat=torch.zeros(pool, q, 2, dtype=torch.long, device=dev),
      rewards=torch.zeros(pool, device=dev),
      perts=torch.full((pool,), 0.16, device=dev))


def test_eagle_suggest_checks_its_arguments(ext):
  call = _Call()
  call.suggest(ext)                    # the unmodified call is valid
  raises = lambda match: pytest.raises(RuntimeError, match=match)
  with raises('pool_cont must be a GPU tensor'):
    call.suggest(ext, pool_cont=call.pool_cont.cpu())
  with raises('rewards must be fp32'):
    call.suggest(ext, rewards=call.rewards.double())
  with raises('perturbations must be fp32'):
    call.suggest(ext, perts=call.perts.double())
  with raises('pool_cat / cat_sizes must be int64 GPU'):
    call.suggest(ext, pool_cat=call.pool_cat.int())
  with raises('pool_cat / cat_sizes must be int64 GPU'):
    call.suggest(ext, cat_sizes=call.cat_sizes.cpu())
  with raises('out_cont must be a contiguous GPU tensor'):
    call.suggest(ext, out_cont=call.out_cont.double())
  wide = torch.empty(25, 1, 6, device='cuda')[:, :, ::2]
  assert wide.shape == call.out_cont.shape and not wide.is_contiguous()
  with raises('out_cont must be a contiguous GPU tensor'):
    call.suggest(ext, out_cont=wide)
  with raises('out_cat must be a contiguous GPU tensor'):
    call.suggest(ext, out_cat=call.out_cat.cpu())
  # 144 = max_pool_size 100 rounded up to a batch size of 48: the kernel
  # would write scale[128 .. 143] over its own reduction scratch.
  with raises('1 <= pool <= 128'):
    call.suggest(ext, **_big_pool(144), n_batches=3, batch=48,
                 out_cont=torch.empty(48, 1, 3, device='cuda'),
                 out_cat=torch.empty(48, 1, 2, dtype=torch.long,
                                     device='cuda'))
  with raises('1 <= pool <= 128'):
    call.suggest(ext, **_big_pool(129))
  with raises('1 <= q <= 16'):
    call.suggest(ext, **_big_pool(50, q=17),
                 out_cont=torch.empty(25, 17, 3, device='cuda'),
                 out_cat=torch.empty(25, 17, 2, dtype=torch.long,
                                     device='cuda'))
  with raises('must not exceed the pool'):
    call.suggest(ext, n_batches=3)
  with raises('must not exceed the pool'):
    call.suggest(ext, n_batches=0)
  with raises('pool shape mismatch'):
    call.suggest(ext, rewards=call.rewards[:-1].contiguous())
  with raises('pool shape mismatch'):
    call.suggest(ext, cat_sizes=call.cat_sizes[:1].contiguous())
  with raises('out_cont / out_cat must be'):
    call.suggest(ext, out_cont=torch.empty(24, 1, 3, device='cuda'))
  with raises('out_cont / out_cat must be'):
    call.suggest(ext, out_cat=torch.empty(25, 1, 1, dtype=torch.long,
                                          device='cuda'))
  with raises('max_cat must be >= 1'):
    call.suggest(ext, max_cat=0)
  with raises('iter_counter must be int64 cuda with >= 2 slots'):
    call.suggest(ext, iter_t=call.iter_t[:1].contiguous())
  with raises('iter_counter must be int64 cuda with >= 2 slots'):
    call.suggest(ext, iter_t=call.iter_t.int())


def test_eagle_update_checks_its_arguments(ext):
  call = _Call()
  before = call.pool_cont.clone()
  raises = lambda match: pytest.raises(RuntimeError, match=match)
  with raises('pool_cont must be a contiguous GPU tensor'):
    call.update(ext, pool_cont=call.pool_cont.double())
  with raises('pool_cont must be a contiguous GPU tensor'):
    call.update(ext, pool_cont=torch.rand(50, 1, 6, device='cuda')[..., ::2])
  with raises('pool_cat must be a contiguous GPU tensor'):
    call.update(ext, pool_cat=call.pool_cat.cpu())
  with raises('rewards must be a contiguous GPU tensor'):
    call.update(ext, rewards=call.rewards.cpu())
  with raises('perturbations must be a contiguous GPU tensor'):
    call.update(ext, perts=call.perts.double())
  with raises('best_reward must be a contiguous GPU tensor'):
    call.update(ext, best=call.best.double())
  with raises('iter_counter must be a contiguous GPU tensor'):
    call.update(ext, iter_t=call.iter_t.int())
  with raises('batch_cont must be fp32'):
    call.update(ext, batch_cont=call.batch_cont.double())
  with raises('batch_rewards must be a GPU tensor'):
    call.update(ext, batch_rewards=call.batch_rewards.cpu())
  with raises('batch_cat / cat_sizes must be int64 GPU'):
    call.update(ext, batch_cat=call.batch_cat.int())
  with raises('1 <= pool <= 128'):
    call.update(ext, **_big_pool(144))
  q17 = _big_pool(50, q=17)
  with raises('1 <= q <= 16'):
    call.update(ext, **q17, batch_cont=torch.rand(25, 17, 3, device='cuda'),
                batch_cat=torch.zeros(25, 17, 2, dtype=torch.long,
                                      device='cuda'))
  with raises('must not exceed the pool'):
    call.update(ext, n_batches=3)
  with raises('pool / batch shape mismatch'):
    call.update(ext, batch_rewards=call.batch_rewards[:-1].contiguous())
  with raises('pool / batch shape mismatch'):
    call.update(ext, batch_cont=torch.rand(25, 1, 4, device='cuda'))
  with raises('pool / batch shape mismatch'):
    call.update(ext, iter_t=call.iter_t[:1].contiguous())
  with raises('pool / batch shape mismatch'):
    call.update(ext, best=call.best[:0])
  # Nothing was launched by any of the rejected calls.
  assert torch.equal(call.pool_cont, before)
  assert call.iter_t.tolist() == [5] * 12


@pytest.mark.parametrize('kwargs', [
    # 40 features reach max_pool_size = 100, rounded up to 3 x 48 = 144.
    dict(n_continuous=40, batch_size=48),
    dict(n_continuous=4, batch_size=25, pool_size=150),   # config.pool_size
    dict(n_continuous=4, batch_size=5, n_parallel=17),
], ids=['batch48', 'pool150', 'q17'])
def test_strategy_beyond_the_kernel_limits_takes_the_torch_path(ext, kwargs):
  from vizier_amd._src.algorithms.optimizers import eagle as eagle_lib
  kwargs = dict(kwargs)
  config = eagle_lib.EagleStrategyConfig(pool_size=kwargs.pop('pool_size', 0))
  s = eagle_lib.VectorizedEagleStrategy(
      categorical_sizes=[3], seed=0, device='cuda', config=config, **kwargs)
  if kwargs['batch_size'] == 48:
    assert s.pool_size == 144
  assert (s.pool_size > eagle_lib.HIP_MAX_POOL or
          s.n_parallel > eagle_lib.HIP_MAX_PARALLEL)
  assert s._ext is None
  state = s.init_state()
  for _ in range(s.pool_size // s.batch_size + 1):   # init + one steady step
    batch = s.suggest(state)
    r = -((batch.continuous - 0.5) ** 2).sum(dim=(1, 2))
    state = s.update(state, batch, r)
  assert bool(torch.isfinite(batch.continuous).all())
  assert bool(torch.isfinite(state.rewards).all())
  # Within the limits the same call constructs the HIP path.
  inside = eagle_lib.VectorizedEagleStrategy(
      n_continuous=4, categorical_sizes=[3], batch_size=5, seed=0,
      device='cuda')
  assert inside._ext is not None
