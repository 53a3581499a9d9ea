"""The cases of tests/accum_ref.py have the properties they are named for, and the case set rejects every way of getting
rigl_grad_accumulate wrong that the contract (include/rigl_hip.h) rules out.  No GPU."""
import numpy as np
import pytest

import accum_ref as R

F32, U32 = R.F32, R.U32
CASES = R.build_cases()
BY_NAME = {c['name']: c for c in CASES}


def _sub(b):
  b = np.asarray(b, dtype=U32)
  return ((b & U32(0x7F800000)) == 0) & ((b & U32(0x007FFFFF)) != 0)


def _col(name):
  c = BY_NAME[name]
  m = c['m']
  assert m >= 7
  return c['g'][0][:m], c['g'][1][:m], c['g'][2][:m]


def test_sizes_cover_every_boundary():
  ns = {c['n'] for c in CASES}
  assert {0, 1, 3, 4, 5} <= ns
  for edge in (R.WAVE, R.TILE, 3 * R.TILE):
    assert {edge - 1, edge, edge + 1} <= ns
  assert R.WAVE == 64 * 4 and R.TILE == 256 * 4 * 4
  from rigl_amd import _lib
  assert R.TILE == _lib.ACC_TILE and (R.FIRST, R.ADD, R.LAST) == (_lib.ACC_FIRST, _lib.ACC_ADD, _lib.ACC_LAST)
  assert any(c['n'] % 4 and c['n'] > R.TILE for c in CASES) and any(c['n'] % 64 for c in CASES)


def test_layout_is_aligned_and_poisoned():
  for c in CASES:
    buf, lay = R.state_before(c, R.FIRST)
    assert lay['acc'] % 64 == 0 and lay['g'] % 64 == 0 and lay['acc'] != lay['g']
    live = np.zeros(lay['total'], dtype=bool)
    for k in ('acc', 'g'):
      live[lay[k]:lay[k] + lay['n']] = True
    for k in ('loss', 'loss_acc', 'loss_mean'):
      live[lay[k]] = True
    assert np.all(buf[~live] == R.POISON) and int(np.sum(~live)) >= 3 * R.GUARD + 5
    assert np.all(buf.view(np.uint8)[np.repeat(~live, 4)] == 0xFF)


def test_signed_zeros_in_every_pairing():
  a, b, c = _col('signed_zeros')
  assert {(int(x), int(y)) for x, y in zip(a, b)} == {(p, q) for p in (0, 0x80000000) for q in (0, 0x80000000)}
  s = R.add32(a, b)
  assert {int(x) for x in s} == {0, 0x80000000}                       # -0 + -0 = -0, every other pairing +0
  assert np.all(s[(a == 0x80000000) & (b == 0x80000000)] == 0x80000000)


def test_subnormal_cases():
  a, b, c = _col('subnormal_sum_subnormal')
  k = len(np.unique(np.stack([a, b, c]), axis=1).T)
  assert np.all(_sub(a) & _sub(b)) and np.all(_sub(R.add32(a, b))) and np.all(_sub(R.add32(R.add32(a, b), c))) and k >= 3
  a, b, c = _col('subnormal_sum_normal')
  s2, s3 = R.add32(a, b), R.add32(R.add32(a, b), c)
  assert np.all(_sub(a) & _sub(b))
  normal = lambda x: (x & U32(0x7F800000)) != 0
  assert np.all(normal(s2) | normal(s3)) and np.any(normal(s2))


def test_overflow_inf_and_nan_cases():
  a, b, c = _col('overflow')
  fin = lambda x: (x & U32(0x7F800000)) != U32(0x7F800000)
  assert np.all(fin(a) & fin(b) & fin(c)) and np.all(~fin(R.add32(a, b)) | ~fin(R.add32(R.add32(a, b), c)))
  assert np.any(~fin(R.add32(a, b)) & ~R.is_nan(R.add32(a, b)))
  a, b, c = _col('inf_minus_inf')
  s3 = R.add32(R.add32(a, b), c)
  assert np.all(~R.is_nan(a) & ~R.is_nan(b) & ~R.is_nan(c)) and np.all(R.is_nan(s3))
  a, b, c = _col('nan')
  assert np.all(R.is_nan(a) | R.is_nan(b) | R.is_nan(c)) and np.all(R.is_nan(R.add32(R.add32(a, b), c)))


def test_order_triples_tell_three_summations_apart():
  a, b, c = _col('order_triples')
  told = 0
  for x, y, z in zip(R.floats(a), R.floats(b), R.floats(c)):
    v = R.order_variants(x, y, z)
    told += len(set(v)) == 3
    assert v[0] == int(R.add32(R.add32(R.bits(x), R.bits(y)), R.bits(z))[0])
  assert told >= 9


def test_loss_triples_tell_three_means_apart():
  seen = set()
  for c in CASES:
    m, d, w = R.loss_variants(*c['loss'])
    assert m != d and m != w
    seen.add(c['loss'])
  assert BY_NAME['loss_triple']['n'] == 0 and len(seen) >= 2


# ---- mutants -----------------------------------------------------------------------------------------------------------------
def _first_adds_into_stale(buf, lay, mode, inv_k, max_blocks):
  R.reference(buf, lay, R.ADD if mode == R.FIRST else mode, inv_k)


def _last_rewrites_acc(buf, lay, mode, inv_k, max_blocks):
  R.reference(buf, lay, mode, inv_k)
  if mode == R.LAST:
    n = lay['n']
    buf[lay['acc']:lay['acc'] + n] = buf[lay['g']:lay['g'] + n]


def _last_leaves_g(buf, lay, mode, inv_k, max_blocks):
  if mode == R.LAST:
    keep = buf[lay['g']:lay['g'] + lay['n']].copy()
    R.reference(buf, lay, mode, inv_k)
    buf[lay['g']:lay['g'] + lay['n']] = keep
  else:
    R.reference(buf, lay, mode, inv_k)


class _Fp64RunningSum:
  """Keeps the sum in fp64 and rounds where it stores."""

  def __init__(self):
    self.s = None

  def __call__(self, buf, lay, mode, inv_k, max_blocks):
    n = lay['n']
    g = R.floats(buf[lay['g']:lay['g'] + n]).astype(np.float64)
    R.reference(buf, lay, mode, inv_k)
    with np.errstate(all='ignore'):
      if mode == R.FIRST:
        self.s = g
      elif mode == R.ADD:
        self.s = self.s + g
      elif self.s is not None and len(self.s) == n:
        buf[lay['g']:lay['g'] + n] = R.bits((self.s + g).astype(F32))


class _RightToLeft:
  """g1 + (g2 + g3)."""

  def __init__(self):
    self.h = []

  def __call__(self, buf, lay, mode, inv_k, max_blocks):
    n = lay['n']
    g = buf[lay['g']:lay['g'] + n].copy()
    R.reference(buf, lay, mode, inv_k)
    if mode == R.FIRST:
      self.h = [g]
    elif mode == R.ADD:
      self.h.append(g)
    elif len(self.h) == 2 and len(self.h[0]) == n:
      buf[lay['g']:lay['g'] + n] = R.add32(self.h[0], R.add32(self.h[1], g))


def _flushes_subnormals(buf, lay, mode, inv_k, max_blocks):
  R.reference(buf, lay, mode, inv_k)
  if mode != R.FIRST:
    dst = lay['g'] if mode == R.LAST else lay['acc']
    v = buf[dst:dst + lay['n']]
    v[_sub(v)] &= U32(0x80000000)


def _drops_the_tail(buf, lay, mode, inv_k, max_blocks):
  n = lay['n']
  dst = lay['g'] if mode == R.LAST else lay['acc']
  keep = buf[dst + n // 4 * 4:dst + n].copy()
  R.reference(buf, lay, mode, inv_k)
  buf[dst + n // 4 * 4:dst + n] = keep


def _stores_one_past_n(buf, lay, mode, inv_k, max_blocks):
  R.reference(buf, lay, mode, inv_k)
  dst = lay['g'] if mode == R.LAST else lay['acc']
  buf[dst + lay['n']] = 0


def _loss_mean_by_division(buf, lay, mode, inv_k, max_blocks):
  s = R.floats(R.add32(buf[lay['loss_acc']:lay['loss_acc'] + 1], buf[lay['loss']:lay['loss'] + 1]))
  R.reference(buf, lay, mode, inv_k)
  if mode == R.LAST:
    buf[lay['loss_mean']] = R.bits(s / F32(round(1.0 / inv_k)))[0]


class _LossMeanFromFp64:
  def __init__(self):
    self.s = 0.0

  def __call__(self, buf, lay, mode, inv_k, max_blocks):
    l = np.float64(R.floats(buf[lay['loss']:lay['loss'] + 1])[0])
    R.reference(buf, lay, mode, inv_k)
    self.s = l if mode == R.FIRST else self.s + l
    if mode == R.LAST:
      buf[lay['loss_mean']] = R.bits(F32(self.s / round(1.0 / inv_k)))[0]


MUTANTS = {
    'first_adds_into_stale_acc': lambda: _first_adds_into_stale,
    'last_rewrites_acc': lambda: _last_rewrites_acc,
    'last_leaves_g': lambda: _last_leaves_g,
    'fp64_running_sum': _Fp64RunningSum,
    'right_to_left': _RightToLeft,
    'flushed_subnormals': lambda: _flushes_subnormals,
    'dropped_tail': lambda: _drops_the_tail,
    'store_one_past_n': lambda: _stores_one_past_n,
    'loss_mean_by_division': lambda: _loss_mean_by_division,
    'loss_mean_rounded_once_from_fp64': _LossMeanFromFp64,
}


def _complaints(make, stages=True):
  out = []
  for c in CASES:
    if stages:
      for mode in R.MODES:
        out += [(c['name'], mode, m) for m in R.check_stage(make(), c, mode)]
    out += [(c['name'], 'chain', m) for m in R.check_chain(make(), c)]
  return out


def test_the_reference_passes_its_own_cases():
  assert _complaints(lambda: R.reference) == []


@pytest.mark.parametrize('name', sorted(MUTANTS))
def test_mutant_is_rejected(name):
  stateful = name in ('fp64_running_sum', 'right_to_left', 'loss_mean_rounded_once_from_fp64')
  got = _complaints(MUTANTS[name], stages=not stateful)        # a stateful mutant only makes sense over a whole chain
  assert got, 'the case set does not reject %s' % name


def test_each_mutant_is_caught_where_expected():
  kinds = lambda name, **kw: {m.split(':')[0] for _, _, m in _complaints(MUTANTS[name], **kw)}
  assert 'untouched' in kinds('last_rewrites_acc') and 'untouched' in kinds('store_one_past_n')
  assert 'value' in kinds('dropped_tail') and 'value' in kinds('right_to_left', stages=False)
  hit = {c for c, _, _ in _complaints(MUTANTS['flushed_subnormals'])}
  assert 'subnormal_sum_subnormal' in hit
  hit = {c for c, _, _ in _complaints(MUTANTS['fp64_running_sum'], stages=False)}
  assert 'order_triples' in hit
