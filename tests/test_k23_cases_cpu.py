"""tests/k23_cases.py checked without a GPU: every case has, in the ORACLE's run, the property it is named for, the
placement helper notices a stray store, and MUTANT oracles -- the update computed the way a subtly wrong kernel would
compute it -- each differ from the true oracle on at least one case of the set.  A mutant that no case rejects means the
set is too soft."""
import numpy as np
import pytest

import k23_cases as K
from oracle import rigl_oracle as O

F32 = np.float32
TINY = np.finfo(F32).tiny


def _bits(a):
  return np.ascontiguousarray(a, F32).reshape(-1).view(np.uint32)


def _has_subnormal(a):
  a = np.abs(np.asarray(a, F32))
  return bool(((a > 0) & (a < TINY)).any())


def _has_neg_zero(a):
  return bool((_bits(a) == 0x80000000).any())


K2 = {c['name']: c for c in K.all_k2_cases()}


# ---- placement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('off', K.OFFSETS)
def test_placement_offsets_guards_and_stray_stores(off):
  ops = dict(w=np.arange(33, dtype=F32), bits=np.arange(2, dtype=np.uint32), sh=np.arange(33, dtype=np.uint16),
             empty=np.zeros(0, F32))
  P = K.Placement(ops, off, offsets=dict(sh=off))
  assert P.guards_intact()
  for name, (start, nb, dt) in P.spans.items():
    want = off if name != 'bits' else 0
    assert (start // dt.itemsize) % (256 // dt.itemsize) == (K.GUARD + want) % (256 // dt.itemsize), name
    np.testing.assert_array_equal(P.views()[name], ops[name])
  spans = sorted(P.spans.values())
  for (s0, n0, d0), (s1, _, d1) in zip(spans, spans[1:]):
    assert s1 - (s0 + n0) >= K.GUARD * (d0.itemsize + d1.itemsize)          # a full guard on each side
  assert spans[0][0] >= K.GUARD * spans[0][2].itemsize
  assert P.nbytes - (spans[-1][0] + spans[-1][1]) >= K.GUARD * spans[-1][2].itemsize
  img = P.buffer.copy()
  P.views(img)['w'][:] = 7                                                   # writing an operand is no guard hit
  assert P.guards_intact(img)
  for name, (start, nb, dt) in P.spans.items():                              # one element before / after each operand is
    for pos in (start - 1, start + nb):
      img = P.buffer.copy()
      img[pos] ^= 0xFF
      assert not P.guards_intact(img), (name, pos)


# ---- the cases have the property they are named for --------------------------------------------------------------------
def test_sizes_cover_the_word_segment_and_chunk_edges():
  for edge in (4, 32, 1024, 4096):
    assert {edge - 1, edge, edge + 1} <= set(K.SIZES)
  assert max(K.SIZES) > 2 * K.CHUNK


@pytest.mark.parametrize('n', [s for s in K.SIZES if s >= 1023])
@pytest.mark.parametrize('noise', [False, True])
def test_size_cases_have_ties_that_straddle_both_thresholds(n, noise):
  c = K.size_case(n, noise, 1)
  r = K.oracle_update(c)
  sd, sg = O.rigl_scores(c['mask'], c['w'], c['g'], c['noise'])
  t1 = sd[r['idx1'][r['n_keep'] - 1]]
  assert 0 < ((sd == t1) & (r['mask1'] == 1)).sum() < (sd == t1).sum()
  lifted = np.where(r['mask1'] == 1, F32(sg.min() - F32(1)), sg)
  t2 = lifted[r['idx2'][r['n_prune'] - 1]]
  assert 0 < ((lifted == t2) & (r['mask2'] == 1)).sum() < (lifted == t2).sum()
  if noise:
    assert (sd[c['mask'] == 0] < 0).any()                                    # negative scores on inactive weights


def test_mode_cases():
  n = K2['frac_zero']['mask'].size
  want = dict(n_ones_zero=(0, 0, 0), dense_mask=None, dense_frac_zero=(n, 0, n), frac_zero=None, frac_one=None, frac_tiny=None)
  for name in want:
    c = K2[name]
    r = K.oracle_update(c)
    assert (r['n_ones'], r['n_prune'], r['n_keep']) == K.expected_counts(c)
    if want[name]:
      assert K.expected_counts(c) == want[name]
  for name in ('frac_zero', 'frac_tiny', 'dense_frac_zero', 'n_ones_zero'):
    assert K.expected_counts(K2[name])[1] == 0                               # n_prune == 0
    assert _bits(K.oracle_update(K2[name])['mask']).tolist() == _bits(K2[name]['mask']).tolist()
  assert K.expected_counts(K2['frac_tiny'])[0] > 0 and K2['frac_tiny']['frac'] > 0
  ones, prune, keep = K.expected_counts(K2['frac_one'])
  assert prune == ones > 0 and keep == 0
  ones, prune, keep = K.expected_counts(K2['dense_mask'])
  assert ones == n and 0 < prune < n
  r = K.oracle_update(K2['dense_mask'])
  assert r['mask'].sum() == n and not r['new_connections'].any()             # every dropped weight regrown, none is new


def test_fp32_count_differs_from_the_double_product():
  c = K2['f32_count']
  ones, prune, _ = K.expected_counts(c)
  assert prune != int(np.float64(ones) * np.float64(F32(c['frac'])))
  assert K.oracle_update(c)['n_prune'] == prune


def test_overlap_case_raises_and_distinct_large_gradients_do_not():
  c = K2['overlap']
  sg = np.abs(c['g'])
  assert F32(sg.min() - F32(1)) == sg.min()
  assert K.oracle_update(c) is None
  with pytest.raises(AssertionError):
    O.rigl_mask_update(c['mask'], c['w'], c['g'], c['frac'], momentum=c['mom'])
  c = K2['large_distinct_grad']
  sg = np.abs(c['g'])
  assert F32(sg.min() - F32(1)) == sg.min() and np.unique(sg).size == sg.size
  assert K.oracle_update(c) is not None


def test_data_cases_plant_what_they_say_and_stay_free_of_nan():
  for c in K.all_k2_cases() + [K.size_case(n, True, 2) for n in K.SIZES]:
    r = K.oracle_update(c)
    if r is None:
      continue
    for a in (r['weights'], r['momentum']):
      assert a is None or not np.isnan(a).any(), c['name']
  c = K2['data_edges']
  sd, sg = O.rigl_scores(c['mask'], c['w'], c['g'], c['noise'])
  assert _has_subnormal(c['w']) and _has_subnormal(c['noise']) and _has_subnormal(c['g']) and _has_subnormal(sd)
  assert np.isposinf(sd).any() and np.isneginf(sd).any() and np.isposinf(sg).any()
  neg = sd[np.isfinite(sd) & (sd < 0)]
  assert np.unique(_bits(neg) >> 21).size > 20                               # many leading radix digits among the negatives
  assert _has_neg_zero(c['g'])
  r = K.oracle_update(c)
  assert np.isfinite(r['weights']).all() and np.isfinite(r['momentum']).all()
  # the negative threshold
  c = K2['negative_threshold']
  r = K.oracle_update(c)
  sd, _ = O.rigl_scores(c['mask'], c['w'], c['g'], c['noise'])
  assert (sd < 0).all() and np.unique(_bits(sd) >> 21).size > 20 and r['n_keep'] > 0
  # grad_sign on +-0 and g * scale on -0: the grown weights are +0 (sign(+-0) = 0), the reset slot carries the sign
  c = K2['grad_sign_zero']
  r = K.oracle_update(c)
  new = r['new_connections']
  assert (c['g'][new] == 0).sum() > 100 and _has_neg_zero(c['g'][new])
  assert not _has_neg_zero(r['weights'][new]) and _has_neg_zero(r['momentum'][new])
  # underflowing products
  c = K2['underflow']
  r = K.oracle_update(c)
  new = r['new_connections']
  assert new.sum() > 100 and _has_subnormal(r['weights'][new]) and _has_subnormal(r['momentum'][new])
  assert _has_subnormal(K.oracle_second_slot(c, r)[new])


def test_score_cases_cut_through_signed_zeros():
  for n in K.SIZES:
    s = K.score_case(n)
    assert not np.isnan(s).any()
    k = K.zero_straddle_k(s)
    if n >= 5:
      assert k is not None and _has_neg_zero(s) and (_bits(s) == 0).any()
      m = K.topk_mask_ref(s, k)
      assert 0 < m[s == 0].sum() < (s == 0).sum()


def test_explicit_score_cases_cut_through_signed_zeros():
  for n in (33, 1025, 4097):
    c, d = K.explicit_score_cases(n)
    r = K.oracle_update_explicit(c)
    sd = c['score_drop']
    assert r['n_prune'] == 0 and 0 < r['mask1'][sd == 0].sum() < (sd == 0).sum()
    assert _has_neg_zero(sd[r['mask1'] == 1]) and (_bits(sd[r['mask1'] == 1]) == 0).any()
    r = K.oracle_update_explicit(d)
    assert r['n_prune'] > 0 and r['new_connections'].any()


def test_layer_table_shape():
  sizes = K.layer_table()
  chunks = sum(-(-n // K.CHUNK) for n in sizes)
  assert len(sizes) == 5000 and chunks > 4096 and sum(sizes) < 4_000_000
  assert sizes[0] == 0 and sizes[-1] == 0 and sizes.count(0) == 3 and 0 in sizes[2400:2600]
  assert sum(1 for n in sizes if n > K.CHUNK) >= 5
  # every capped grid (1536 / 2048 / 4096 workgroups) has a range that holds a complete layer between two others, and
  # one whose range holds a zero-length entry of the table strictly inside
  first = np.concatenate([[0], np.cumsum([-(-n // K.CHUNK) for n in sizes])])
  for wgs in K.GRID_CAPS:
    inner = zero_inside = 0
    for b in range(wgs):
      c0, c1 = b * chunks // wgs, (b + 1) * chunks // wgs
      ls = [l for l in range(np.searchsorted(first, c0, 'right') - 1, len(sizes)) if first[l] < c1 and first[l + 1] > c0] \
          if c1 > c0 else []
      inner += len(ls) >= 3
      zero_inside += any(sizes[l] == 0 and c0 < first[l] < c1 for l in range(len(sizes)) if sizes[l] == 0)
    assert inner > 0 and zero_inside > 0, (wgs, inner, zero_inside)
  t = K.table_case(sizes)
  assert t['w'].size == sum(sizes) and len({int(a) % 4 for a in t['start'][:-1]}) == 4      # bases at every alignment


def test_momentum_inputs_hold_every_signed_zero_combination():
  w, g, a, mask = K.momentum_inputs(4097)
  for arr in (w, g, a):
    assert not np.isnan(arr).any()
    for on in (0, 1):
      assert _has_neg_zero(arr[mask == on]) and (_bits(arr[mask == on]) == 0).any()
  # the case of the issue: a = -0.0, mask off, g < 0, w < 0
  assert ((_bits(a) == 0x80000000) & (mask == 0) & (g < 0) & (w < 0)).any()
  assert _has_subnormal(a)
  lrs, mus, wds, gss, nes = [set(x) for x in zip(*K.MOMENTUM_GRID)]
  assert 0.0 in lrs and {0.0, 1.0} <= mus and 0.0 in wds and len(wds) > 1 and gss == {1.0, 0.125} and nes == {True, False}
  for mk in (mask, None):
    for cfg in K.MOMENTUM_GRID:
      w1, a1, _ = K.momentum_ref(w, g, a, mk, *cfg)
      assert not np.isnan(w1).any() and not np.isnan(a1).any()
  w1, a1, _ = K.momentum_ref(w, g, a, mask, 0.1, 0.9, 0.0, 1.0, True)
  assert _has_neg_zero(a1[mask == 0])                                        # the -0.0 momentum survives a masked-off step


# ---- mutants --------------------------------------------------------------------------------------------------------------
def _ftz(a):
  a = np.asarray(a, F32)
  return np.where(np.abs(a) < TINY, np.copysign(F32(0), a), a).astype(F32)


def _order(x, high_index=False, negzero_below=False):
  """tf.nn.top_k's order; the mutants: equal values by HIGHER index, -0.0 below +0.0."""
  x = np.asarray(x)
  if negzero_below:
    b = np.asarray(x, F32).view(np.uint32)
    key = np.uint32(0xFFFFFFFF) - np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
  else:
    key = -x
  if high_index:
    return (x.size - 1 - np.argsort(key[::-1], kind='stable')).astype(np.int32)
  return np.argsort(key, kind='stable').astype(np.int32)


def _update(c, high_index=False, negzero_below=False, nprune_double=False, lifted_double=False, ftz=False):
  """get_update + the RigL scores and grow tensors, restated with one switch per mutant.  No switch: the oracle."""
  z = _ftz if ftz else (lambda a: np.asarray(a, F32))
  with np.errstate(all='ignore'):
    mask, w, g = c['mask'], z(c['w']), z(c['g'])
    sd = z(np.abs(mask * w))
    if c['noise'] is not None:
      sd = z((sd + z(c['noise'])).astype(F32))
    sg = np.abs(g)
    n_ones = np.int32(np.sum(mask, dtype=F32))
    if nprune_double:
      n_prune = np.int32(np.float64(n_ones) * np.float64(F32(c['frac'])))
    else:
      n_prune = np.int32(F32(F32(n_ones) * F32(c['frac'])))
    n_keep = np.int32(n_ones - n_prune)
    mask1 = np.zeros(mask.size, F32)
    mask1[_order(sd, high_index, negzero_below)[:max(int(n_keep), 0)]] = 1
    if lifted_double:
      lifted = np.where(mask1 == 1, np.float64(sg.min()) - 1.0, sg.astype(np.float64))
    else:
      lifted = np.where(mask1 == 1, F32(sg.min() - F32(1)), sg).astype(F32)
    mask2 = np.zeros(mask.size, F32)
    mask2[_order(lifted, high_index, negzero_below and not lifted_double)[:max(int(n_prune), 0)]] = 1
    if (mask1 * mask2).sum() != 0:
      return None
    new = (mask2 == 1) & (mask == 0)
    d = F32(O.extract_number(c['grow_init']))
    if c['grow_init'].startswith('grad_scale'):
      grow = z((g / d).astype(F32))
    elif c['grow_init'].startswith('grad_sign'):
      grow = z((np.sign(g) / d).astype(F32))
    else:
      grow = np.zeros_like(w)
    out = dict(mask=mask1 + mask2, weights=np.where(new, grow, c['w']).astype(F32), n_prune=int(n_prune), momentum=None)
    if c['mom'] is not None:
      out['momentum'] = np.where(new, z((g * F32(c['acc_scale'])).astype(F32)), c['mom']).astype(F32)
    return out


def _same_update(a, b):
  if a is None or b is None:
    return a is None and b is None
  return all((a[k] is None and b[k] is None) or np.array_equal(_bits(a[k]), _bits(b[k])) for k in ('mask', 'weights', 'momentum'))


def _all_update_cases():
  return K.all_k2_cases() + [K.size_case(n, noise, 1) for n in K.SIZES for noise in (False, True)]


def test_the_restated_update_without_a_switch_is_the_oracle():
  for c in _all_update_cases():
    assert _same_update(_update(c), K.oracle_update(c)), c['name']
  for n in K.SIZES:
    s = K.score_case(n)
    np.testing.assert_array_equal(_order(s), O.topk_order(s))


@pytest.mark.parametrize('switch', ['high_index', 'nprune_double', 'lifted_double', 'ftz'])
def test_update_mutants_are_rejected(switch):
  bad = [c['name'] for c in _all_update_cases() if not _same_update(_update(c, **{switch: True}), K.oracle_update(c))]
  print(switch, 'rejected by', bad)
  assert bad, 'no case rejects the mutant "%s"' % switch
  if switch == 'nprune_double':
    assert 'f32_count' in bad
  if switch == 'lifted_double':
    assert 'overlap' in bad
  if switch == 'ftz':
    assert {'data_edges', 'underflow'} <= set(bad)


@pytest.mark.parametrize('switch', ['high_index', 'negzero_below'])
def test_topk_mutants_are_rejected(switch):
  bad = []
  for n in K.SIZES:
    s = K.score_case(n)
    for k in {1, n, K.zero_straddle_k(s) or 1}:
      m = np.zeros(n, F32)
      m[_order(s, **{switch: True})[:k]] = 1
      if not np.array_equal(m, K.topk_mask_ref(s, k)):
        bad.append((n, k))
  assert bad, 'no score case rejects the mutant "%s"' % switch
  assert {n for n, _ in bad} >= {n for n in K.SIZES if n >= 31}              # every size beyond a few elements does


def _momentum_mutant(w, g, a, mask, lr, mu, wd, gs, nesterov, fma=False, select=False):
  with np.errstate(all='ignore'):
    if select:                      # (mask ? grad_scale * g : 0), the decay term skipped when wd == 0
      gm = g if F32(gs) == F32(1) else (g * F32(gs)).astype(F32)
      gm = np.where(mask != 0, gm, F32(0)).astype(F32)
      gv = (gm + (F32(wd) * w).astype(F32)).astype(F32) if F32(wd) != F32(0) else gm
    else:
      gv = K.unified_masked_grad(g, mask, w, wd, gs)
    if not fma:
      return O.momentum_apply(w, a, gv, lr, mu, nesterov=nesterov)
    a1 = (a.astype(np.float64) * np.float64(F32(mu)) + gv.astype(np.float64)).astype(F32)       # one rounding
    return O.momentum_apply(w, a, gv, lr, mu, nesterov=nesterov)[0], a1


@pytest.mark.parametrize('switch', ['fma', 'select'])
def test_momentum_mutants_are_rejected(switch):
  w, g, a, mask = K.momentum_inputs(4097)
  bad = []
  for cfg in K.MOMENTUM_GRID:
    w0, a0, _ = K.momentum_ref(w, g, a, mask, *cfg)
    w1, a1 = _momentum_mutant(w, g, a, mask, *cfg, **{switch: True})
    if not (np.array_equal(_bits(w0), _bits(w1)) and np.array_equal(_bits(a0), _bits(a1))):
      bad.append(cfg)
  assert bad, 'no grid point rejects the mutant "%s"' % switch
  if switch == 'select':
    assert any(cfg[2] == 0.0 for cfg in bad) and any(cfg[2] != 0.0 for cfg in bad)       # with and without decay
