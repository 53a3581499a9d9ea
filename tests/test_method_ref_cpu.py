"""tests/method_ref.py checked on its own (no GPU): the reference's unit-test statements hold on it, every case has the
property it is named for, and the case set tells every mutant order of operations from the reference.

Workload: a three-layer arena table -- 'a' 40x50 at sparsity 0.98, 'b' 5x2 (10 elements) at 0.5, 'c' 30x10 at 0 -- with
64-element slot padding, a dense-kernel segment and a BN / bias segment, l2 5e-4 on the kernels, driven by seeded
synthetic gradient sequences.  Everything is bit equality; no tolerance appears."""
import functools

import numpy as np
import pytest

import method_ref as R
from oracle import rigl_oracle as O

F32 = np.float32
WD = 5e-4
CALLS = 8
SPARSITY = {'a': 0.98, 'b': 0.5, 'c': 0.0}


def _arena():
  layers, off = [], 0
  for scope, shape in (('a', (40, 50)), ('b', (5, 2)), ('c', (30, 10))):
    layers.append(R.Layer(scope, off, shape))
    off += (layers[-1].numel + 63) // 64 * 64
  n_masked, n_kernel, total = off, off + 128, off + 128 + 64
  wd = np.zeros(total, F32)
  wd[:n_kernel] = WD
  return R.Arena(total, n_masked, n_kernel, wd, layers)


ARENA = _arena()
DENSE = slice(ARENA.n_masked, ARENA.n_masked + 100)       # one dense kernel of 100 weights
OTHER = slice(ARENA.n_kernel, ARENA.n_kernel + 40)        # BN / bias


def _fill(rs, scale):
  """Values on the variables, zeros in the padding (as the device's arena)."""
  x = np.zeros(ARENA.total, F32)
  for sl in [l.sl for l in ARENA.layers] + [DENSE, OTHER]:
    x[sl] = (rs.standard_normal(sl.stop - sl.start) * scale).astype(F32)
  return x


def _start(seed, dense_masks=False, spread=False):
  rs = np.random.RandomState(seed)
  W = _fill(rs, 0.1)
  if spread:                  # magnitudes from 1e-7 up: the drop threshold falls where the 1e-5 noise decides the ranking
    a = ARENA.layers[0]
    W[a.sl] = (W[a.sl] * 10.0 ** rs.uniform(-6, 0, a.numel)).astype(F32)
  mask = np.zeros(ARENA.n_masked, F32)
  for l in ARENA.layers:
    mask[l.sl] = 1 if dense_masks else O.get_mask_random_numpy([l.numel], SPARSITY[l.scope], rs)
  return W, mask


def _grads(seed, scale=0.3):
  rs = np.random.RandomState(1000 + seed)
  return [_fill(rs, scale) for _ in range(CALLS)]


def _dyn(method, inner, **kw):
  kw.setdefault('begin', 1)
  kw.setdefault('end', 100)
  kw.setdefault('frequency', 3)
  kw.setdefault('drop_fraction', 0.3)
  return R.Cfg(method, inner, lr=0.1 if inner != 'adam' else 0.01, **kw)


MAP = dict(SPARSITY)
CASES = {
    'set-sgd': (_dyn('set', 'sgd'), {}),
    'set-momentum': (_dyn('set', 'momentum'), {}),
    'set-adam': (_dyn('set', 'adam'), {}),
    'static-momentum': (_dyn('static', 'momentum'), {}),
    'static-adam': (_dyn('static', 'adam'), {}),
    'snfs-sgd': (_dyn('snfs', 'sgd'), {}),
    'snfs-momentum': (_dyn('snfs', 'momentum'), {}),
    'snfs-adam': (_dyn('snfs', 'adam'), {}),
    'rigl-momentum': (_dyn('rigl', 'momentum', begin=0, initial_acc_scale=0.5), dict(spread=True)),
    'rigl-adam-grad_scale': (_dyn('rigl', 'adam', begin=0, grow_init='grad_scale_2'), {}),
    'rigl-momentum-grad_sign': (_dyn('rigl', 'momentum', begin=0, grow_init='grad_sign_4'), {}),
    'rigl-momentum-uniform': (_dyn('rigl', 'momentum', begin=0, grow_init='random_uniform_2'), {}),
    'rigl-adam-normal': (_dyn('rigl', 'adam', begin=0, grow_init='random_normal_2'), {}),
    'snip-momentum-l2': (R.Cfg('snip', 'momentum', lr=0.1, default_sparsity=0.5), dict(dense_masks=True, gscale=0.002)),
    'snip-momentum-map': (R.Cfg('snip', 'momentum', lr=0.1, default_sparsity=0.5, custom_sparsity_map=MAP), dict(dense_masks=True)),
    'dnw-sgd': (R.Cfg('dnw', 'sgd', lr=0.1, default_sparsity=0.5, custom_sparsity_map=MAP), {}),
    'dnw-momentum': (R.Cfg('dnw', 'momentum', lr=0.1, default_sparsity=0.5, custom_sparsity_map=MAP), {}),
}
MUTANT_CASE = {
    'set_update_on_pre_apply_weights': 'set-sgd', 'seed_step_before_increment': 'set-sgd', 'grow_drop_tags_swapped': 'set-sgd',
    'signed_ema_grow_score': 'snfs-sgd', 'ema_updated_after_the_update': 'snfs-momentum', 'ema_of_masked_gradient': 'snfs-adam',
    'static_without_reinit': 'static-momentum', 'rigl_momentum_reset_in_set': 'set-momentum',
    'second_adam_slot_not_reset': 'set-adam', 'dnw_l2_on_masked_kernels': 'dnw-sgd', 'dnw_masked_gradient': 'dnw-momentum',
    'dnw_no_l2_on_dense_kernels': 'dnw-sgd', 'dnw_scores_shifted_by_one': 'dnw-momentum',
    'snip_score_without_wd': 'snip-momentum-l2', 'snip_increments_step': 'snip-momentum-map',
    'rigl_applies_on_update_call': 'rigl-adam-grad_scale', 'drop_noise_left_out': 'rigl-momentum',
}


@functools.lru_cache(maxsize=None)
def _run(case, mutant=None):
  """The trajectory of a case: [(state before, G, state after, info)] of CALLS calls; computed once, never modified."""
  cfg, how = CASES[case]
  how = dict(how)
  gscale = how.pop('gscale', 0.3)
  seed = sorted(CASES).index(case)
  W, mask = _start(seed, **how)
  st = R.initial_state(cfg, ARENA, W, mask)
  out = []
  for G in _grads(seed, gscale):
    new, info = R.step(cfg, ARENA, st, G, mutant=mutant)
    out.append((st, G, new, info))
    st = new
  return out


_compared = R.compared


def _updates(traj):
  return [(i, t) for i, t in enumerate(traj) if t[3]['is_update']]


# ---------------------------------------------------------------------------------------------- (c) the mutants
def test_every_mutant_has_a_case():
  assert set(MUTANT_CASE) == set(R.MUTANTS) and len(R.MUTANTS) == 17


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_case_set_rejects_the_mutant(mutant):
  case = MUTANT_CASE[mutant]
  ref, mut = _run(case), _run(case, mutant)
  differs = any(R.outcomes_differ(a, ia, b, ib) for (_, _, a, ia), (_, _, b, ib) in zip(ref, mut))
  assert differs, '%s is not told from the reference by case %s' % (mutant, case)


def test_the_reference_is_a_pure_function():
  """Same inputs, same outputs; and no input array is modified."""
  cfg, how = CASES['set-adam']
  W, mask = _start(3, **how)
  st = R.initial_state(cfg, ARENA, W, mask)
  G = _grads(3)[0]
  for _ in range(3):
    st, _ = R.step(cfg, ARENA, st, G)
  keep = [x.copy() for x in _compared(st, dict(drop_fraction=None, counts=None))] + [G.copy()]
  a, ia = R.step(cfg, ARENA, st, G)
  b, ib = R.step(cfg, ARENA, st, G)
  assert ia['is_update']
  assert all(R.first_diff(x, y) is None for x, y in zip(_compared(a, ia), _compared(b, ib)))
  assert all(R.first_diff(x, y) is None for x, y in zip(keep, _compared(st, dict(drop_fraction=None, counts=None)) + [G]))


# ---------------------------------------------------------------------------------------------- (b) the properties
@pytest.mark.parametrize('case', [c for c in sorted(CASES) if CASES[c][0].method in R.SET_FAMILY + ('rigl',)])
def test_dynamic_case_has_its_properties(case):
  cfg = CASES[case][0]
  ups = _updates(_run(case))
  assert len(ups) >= 2 and any(b[0] - a[0] > 1 for a, b in zip(ups, ups[1:]))      # training between two updates
  for _, (_, _, _, info) in ups:
    facts = info['facts']
    assert sum(f['n_prune'] >= 1 for f in facts) >= 2
    if cfg.method == 'static':
      assert sum(f['reinit'] for f in facts) >= 1 and not any(f['mask_changed'] for f in facts)
    else:
      assert sum(f['grown'] for f in facts) >= 1
    assert [int(c[4]) for c in info['counts']] == [0] * len(facts)                 # base:320-321 would not fire
    assert [int(c[7]) for c in info['counts']] == [int(c[0]) for c in info['counts']]


@pytest.mark.parametrize('case', ['dnw-sgd', 'dnw-momentum'])
def test_dnw_case_has_its_properties(case):
  traj = _run(case)
  assert any(f['mask_changed'] for t in traj for f in t[3]['facts'])
  moved = 0
  for st, _, new, _ in traj:
    off = st['mask'] == 0
    for l in ARENA.layers:
      o = off[l.sl]
      moved += int((st['W'][l.sl][o] != new['W'][l.sl][o]).sum())
  assert moved > 0


def test_snip_l2_changes_the_kept_set():
  a = _run('snip-momentum-l2')[0][2]['mask']
  b = _run('snip-momentum-l2', 'snip_score_without_wd')[0][2]['mask']
  assert a.sum() == b.sum() and not np.array_equal(a, b)


def test_drop_noise_changes_an_update():
  a, b = _run('rigl-momentum'), _run('rigl-momentum', 'drop_noise_left_out')
  assert any(not np.array_equal(x[2]['mask'], y[2]['mask']) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- (a) the reference's unit tests
def _toy(method, inner='sgd', **kw):
  """The schedule of sparse_optimizers_test.py's _setup_graph (:40-69): begin 1, end 4, frequency 2."""
  kw.setdefault('begin', 1)
  kw.setdefault('end', 4)
  kw.setdefault('frequency', 2)
  cfg = R.Cfg(method, inner, lr=0.1, **kw)
  W, mask = _start(7)
  return cfg, R.initial_state(cfg, ARENA, W, mask), _grads(7)


@pytest.mark.parametrize('drop_frac', [0.5, 0.2])
def test_set_mask_changes_on_update_iterations_only(drop_frac):
  # sparse_optimizers_test.py:71-92 and :94-118: iterations 1 and 3 update, connections are conserved
  cfg, st, grads = _toy('set', drop_fraction=drop_frac)
  for i, G in enumerate(grads[:5], start=1):
    new, info = R.step(cfg, ARENA, st, G)
    assert info['is_update'] == (i in (1, 3))
    if i in (1, 3):
      assert not np.array_equal(new['mask'], st['mask'])
      for l in ARENA.layers:
        assert new['mask'][l.sl].sum() == st['mask'][l.sl].sum()
    else:
      assert np.array_equal(new['mask'], st['mask'])
    st = new


@pytest.mark.parametrize('begin,end,freq', [(3, 7, 2), (1, 5, 3), (0, 4, 1)])
def test_set_no_drop(begin, end, freq):
  # :120-139
  cfg, st, grads = _toy('set', drop_fraction=0, begin=begin, end=end, frequency=freq)
  for G in grads:
    new, _ = R.step(cfg, ARENA, st, G)
    assert np.array_equal(new['mask'], st['mask'])
    st = new


def test_set_new_connections_start_at_zero():
  # :141-156
  cfg, st, grads = _toy('set', drop_fraction=0.5, begin=0, end=4, frequency=1)
  grown = 0
  for G in grads[:5]:
    new, _ = R.step(cfg, ARENA, st, G)
    born = np.logical_and(st['mask'] == 0, new['mask'] == 1)
    grown += int(born.sum())
    assert np.all(new['W'][:ARENA.n_masked][born] == 0)
    st = new
  assert grown > 0


@pytest.mark.parametrize('drop_frac', [0.5, 0.2])
def test_static_mask_never_changes(drop_frac):
  # :225-244
  cfg, st, grads = _toy('static', drop_fraction=drop_frac)
  for G in grads[:5]:
    new, _ = R.step(cfg, ARENA, st, G)
    assert np.array_equal(new['mask'], st['mask'])
    st = new


@pytest.mark.parametrize('momentum', [0.5, 0., 1.])
def test_snfs_moving_average(momentum):
  # :275-294: ema = ema * momentum + (1 - momentum) * grad.  The gradient is the test's arange, a small integer: for these
  # three decays both forms are exact in fp32, so equality is asserted where the reference's test says close.
  cfg, st, _ = _toy('snfs', ema_decay=momentum, drop_fraction=0.5)
  G = np.zeros(ARENA.total, F32)
  for l in ARENA.layers:
    G[l.sl] = np.arange(l.numel, dtype=F32) % 8
  cur = {l.name: np.zeros(l.numel, F32) for l in ARENA.layers}
  for _ in range(6):
    st, _ = R.step(cfg, ARENA, st, G)
    for l in ARENA.layers:
      cur[l.name] = (cur[l.name] * F32(momentum) + F32(1 - momentum) * G[l.sl]).astype(F32)
      assert np.array_equal(st['ema'][l.name], cur[l.name])


@pytest.mark.parametrize('begin,end,freq,is_incremented', [
    (3, 7, 2, [1, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1]),
    (1, 5, 3, [1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1]),
    (0, 4, 1, [0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 1])])
def test_rigl_global_step_golden(begin, end, freq, is_incremented):
  # :349-367
  cfg, st, grads = _toy('rigl', drop_fraction=0.5, begin=begin, end=end, frequency=freq)
  for i, one in enumerate(is_incremented):
    new, info = R.step(cfg, ARENA, st, grads[i % CALLS])
    assert new['gs'] == st['gs'] + one and info['is_update'] == (not one) and info['applied'] == bool(one)
    st = new


@pytest.mark.parametrize('s', [0.5, 0.8])
def test_snip(s):
  # :404-468
  cfg = R.Cfg('snip', 'sgd', lr=1e-3, default_sparsity=s)
  W, mask = _start(11, dense_masks=True)
  st = R.initial_state(cfg, ARENA, W, mask)
  grads = _grads(11)
  assert all(st['mask'][l.sl].all() for l in ARENA.layers)                     # testInitialMaskIsDense
  new, info = R.step(cfg, ARENA, st, grads[0])
  assert info['is_update'] and new['gs'] == 0 and new['is_snipped']
  assert np.array_equal(new['W'], st['W'])                                     # no gradient applied on the snip call
  for l in ARENA.layers:
    m = new['mask'][l.sl]
    assert l.numel - m.sum() == O.get_n_zeros(l.numel, s)                      # testSnipSparsity
    g = O.masked_grad(grads[0][l.sl], np.ones(l.numel, F32), W[l.sl], WD)      # testGradientUsed (the loss's, l2 included)
    scores = np.abs((g * W[l.sl]).astype(F32))
    assert scores[m == 0].max() <= scores[m == 1].min()
  st = new
  for i in range(3):                                                           # testAfterSnipTraining
    assert st['gs'] == i
    new, info = R.step(cfg, ARENA, st, grads[i + 1])
    assert info['applied'] and np.array_equal(new['mask'], st['mask']) and not np.array_equal(new['W'], st['W'])
    st = new


@pytest.mark.parametrize('s', [0.5, 0.8])
def test_dnw(s):
  # :509-586
  cfg = R.Cfg('dnw', 'sgd', lr=0.1, default_sparsity=s)
  W, mask = _start(13)
  st = R.initial_state(cfg, ARENA, W, mask)
  for G in _grads(13)[:6]:
    new, _ = R.step(cfg, ARENA, st, G)
    for l in ARENA.layers:
      m, w = new['mask'][l.sl], new['W'][l.sl]
      assert l.numel - m.sum() == O.get_n_zeros(l.numel, s)                    # testSparsityAfterDNWUpdates
      assert np.abs(w[m == 0]).max() <= np.abs(w[m == 1]).min()                # testDNWUpdates
      # testGradientIsDense: w -= lr * G on every element, masked-off ones included, and no l2
      assert np.array_equal(w, O.sgd_apply(st['W'][l.sl], G[l.sl], 0.1))
    d = DENSE                                                                  # the dense kernel keeps its l2
    assert np.array_equal(new['W'][d], O.sgd_apply(st['W'][d], O.masked_grad(G[d], np.ones(100, F32), st['W'][d], WD), 0.1))
    assert new['gs'] == st['gs'] + 1
    st = new


# ---------------------------------------------------------------------------------------------- the reduction bound
@pytest.mark.parametrize('n', [10, 512, 1000, 36864])
def test_reduction_bound_admits_fp32_orders_and_separates_the_faults(n):
  """method_ref.reduction_bound: fp32 reductions in three orders (sequential, pairwise, reversed) stay inside it; at the
  small layer sizes of the GPU cases Bessel's correction, a reduction over mask * W and one over the padded slot do not."""
  rs = np.random.RandomState(n)
  w = (rs.standard_normal(n) * 0.05).astype(F32)
  mean64, std64 = float(np.mean(np.abs(w.astype(np.float64)))), float(np.std(w.astype(np.float64)))
  bound = R.reduction_bound(n)

  def seq(x):
    acc = F32(0)
    for v in x:
      acc = F32(acc + v)
    return acc

  a = np.abs(w)
  for total in (seq(a), seq(a[::-1]), np.sum(a, dtype=F32)):
    assert abs(float(F32(total / F32(n))) - mean64) <= bound * mean64
  m = F32(np.sum(w, dtype=F32) / F32(n))
  sq = ((w - m).astype(F32) ** 2).astype(F32)
  for total in (seq(sq), seq(sq[::-1]), np.sum(sq, dtype=F32)):
    assert abs(float(np.sqrt(F32(total / F32(n)))) - std64) <= bound * std64
  if n <= 1000:
    assert abs(float(np.std(w.astype(np.float64), ddof=1)) - std64) > bound * std64           # Bessel's correction
    mask = rs.rand(n) < 0.5
    assert abs(float(np.mean(np.abs(w * mask))) - mean64) > bound * mean64                   # over mask * W
    padded = (n + 63) // 64 * 64
    if padded != n:
      assert abs(float(np.sum(np.abs(w.astype(np.float64))) / padded) - mean64) > bound * mean64   # over the padded slot
