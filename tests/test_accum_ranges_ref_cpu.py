"""The cases of tests/accum_ranges_ref.py have the properties they are named for, and the case set rejects every way of getting
rigl_grad_accumulate_ranges wrong that the contract (include/rigl_hip.h) rules out.  No GPU."""
import os
import re

import numpy as np
import pytest

import accum_ref as A
import accum_ranges_ref as R

U32 = R.U32
CASES = R.build_cases()
BY_NAME = {c['name']: c for c in CASES}


def test_names_are_unique_and_the_constants_agree_with_the_library():
  assert len(BY_NAME) == len(CASES)
  from rigl_amd import _lib
  assert R.MAX_RANGES == _lib.ACC_MAX_RANGES and R.TILE == _lib.ACC_TILE
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  txt = open(os.path.join(root, 'include', 'rigl_hip.h')).read()
  assert int(re.search(r'#define RIGL_ACC_MAX_RANGES (\d+)', txt).group(1)) == R.MAX_RANGES
  assert 'rigl_grad_accumulate_ranges' in _lib.SIGNATURES
  import ctypes
  assert ctypes.sizeof(_lib.AccRange) == 16 and _lib.AccRange.length.offset == 8


def test_every_table_is_legal():
  for c in CASES:
    end = 0
    assert len(c['ranges']) <= R.MAX_RANGES
    for off, ln in c['ranges']:
      assert off % 4 == 0 and ln >= 0 and off >= end and off + ln <= c['n'], c['name']
      end = off + ln


def test_lengths_and_range_counts_are_covered():
  assert R.LENGTHS == (0, 1, 3, 4, 5, 4095, 4096, 4097)
  for ln in R.LENGTHS:
    for kind in ('inside', 'to_n'):
      c = BY_NAME['one_%d_%s' % (ln, kind)]
      assert c['ranges'] == [(8, ln)] and (c['n'] == 8 + ln) == (kind == 'to_n')
  assert {len(c['ranges']) for c in CASES} >= {0, 1, 2, 8}
  for name in ('eight_every_length', 'eight_every_length_reversed'):
    assert sorted(ln for _, ln in BY_NAME[name]['ranges']) == sorted(R.LENGTHS)
  assert sum(ln for _, ln in BY_NAME['head_and_tail']['ranges']) > 5 * R.TILE       # more tiles than the grid caps 1 and 3
  c = BY_NAME['short_then_long']                                                     # whole tiles that start off a tile boundary
  assert c['ranges'][1][0] % R.TILE != 0 and c['ranges'][1][1] > 3 * R.TILE


def _gaps(c):
  r = c['ranges']
  return [r[i + 1][0] - (r[i][0] + r[i][1]) for i in range(len(r) - 1)]


def test_touching_ranges_gaps_of_four_and_a_range_that_ends_at_n():
  assert _gaps(BY_NAME['two_touching']) == [0] and _gaps(BY_NAME['two_touching_to_n']) == [0]
  assert _gaps(BY_NAME['eight_touching']) == [0] * 7 and any(ln == 0 for _, ln in BY_NAME['eight_touching']['ranges'])
  assert _gaps(BY_NAME['eight_gap4'])[0] == 4 and 4 in _gaps(BY_NAME['eight_every_length_reversed'])
  c = BY_NAME['two_gap4']
  off, ln = c['ranges'][0]
  assert c['ranges'][1][0] == -(-(off + ln) // 4) * 4 + 4                           # four whole elements behind the padded end
  assert all(4 <= x < 8 for x in _gaps(BY_NAME['eight_gap4']))
  for name in ('two_touching_to_n', 'eight_every_length', 'eight_touching', 'head_and_tail'):
    c = BY_NAME[name]
    assert sum(c['ranges'][-1]) == c['n'], name
  for name in ('two_touching', 'two_gap4', 'eight_gap4', 'eight_every_length_reversed'):
    c = BY_NAME[name]
    assert sum(c['ranges'][-1]) < c['n'], name


def test_everything_outside_the_ranges_is_poison_in_both_arenas():
  for c in CASES:
    for mode in R.MODES:
      buf, lay = R.state_before(c, mode)
      live = np.zeros(lay['total'], dtype=bool)
      m = R.inside_mask(c['n'], c['ranges'])
      for k in ('acc', 'g'):
        live[lay[k]:lay[k] + c['n']] = m
      for k in ('loss', 'loss_acc', 'loss_mean'):
        live[lay[k]] = True
      assert np.array_equal(buf[~live], R.poisoned(lay)[~live]), (c['name'], mode)
      assert int(np.sum(~live)) >= 3 * A.GUARD + 5
  c = BY_NAME['eight_gap4']
  assert int(np.sum(~R.inside_mask(c['n'], c['ranges']))) >= 7 * 4


def test_special_values_are_where_the_names_say():
  def col(name):
    c = BY_NAME[name]
    idx = np.flatnonzero(R.inside_mask(c['n'], c['ranges']))[:len(c['special'])]
    assert len(idx) >= 7 and len(c['ranges']) == 2 and idx[3] - idx[2] > 1          # the column crosses the gap
    return c['g'][0][idx], c['g'][1][idx], c['g'][2][idx]
  sub = lambda b: ((b & U32(0x7F800000)) == 0) & ((b & U32(0x007FFFFF)) != 0)
  inf = lambda b: (b & U32(0x7FFFFFFF)) == U32(0x7F800000)
  a, b, _ = col('specials_signed_zeros')
  assert {(int(x), int(y)) for x, y in zip(a, b)} == {(p, q) for p in (0, 0x80000000) for q in (0, 0x80000000)}
  a, b, c = col('specials_subnormal_sum_subnormal')
  assert np.all(sub(a) & sub(b)) and np.all(sub(A.add32(A.add32(a, b), c)))
  a, b, c = col('specials_inf_minus_inf')
  assert np.any(inf(a) & (a >> 31 == 0)) and np.any(inf(a) & (a >> 31 == 1)) and np.all(A.is_nan(A.add32(A.add32(a, b), c)))
  a, b, c = col('specials_nan')
  payloads = {int(x) for x in np.concatenate([a, b, c]) if A.is_nan(np.array([x], dtype=U32))[0]}
  assert len(payloads) >= 3 and np.all(A.is_nan(A.add32(A.add32(a, b), c)))       # several NaN payloads; FIRST must copy them
  a, b, c = col('specials_overflow')
  assert np.any(inf(A.add32(a, b)))
  c = BY_NAME['specials_two_odd']
  assert all(ln % 2 == 1 or ln % 4 for _, ln in c['ranges'][:1]) and len(c['special']) > 30


def test_loss_triples_tell_the_roundings_apart():
  seen = set()
  for c in CASES:
    m, d, w = A.loss_variants(*c['loss'])
    assert m != d and m != w and m != R.fused_mean(*c['loss'])
    seen.add(c['loss'])
  assert len(seen) >= 2 and BY_NAME['empty_table_with_loss']['ranges'] == []


# ---- mutants -----------------------------------------------------------------------------------------------------------------
def _end_one_past(buf, lay, ranges, mode, inv_k, max_blocks):
  R.reference(buf, lay, [(o, l + 1) for o, l in ranges], mode, inv_k)


def _end_one_short(buf, lay, ranges, mode, inv_k, max_blocks):
  R.reference(buf, lay, [(o, max(l - 1, 0)) for o, l in ranges], mode, inv_k)


def _second_range_skipped(buf, lay, ranges, mode, inv_k, max_blocks):
  R.reference(buf, lay, ranges[:1] + ranges[2:], mode, inv_k)


def _tail_dropped(buf, lay, ranges, mode, inv_k, max_blocks):
  R.reference(buf, lay, [(o, l // 4 * 4) for o, l in ranges], mode, inv_k)


def _loss_per_range(buf, lay, ranges, mode, inv_k, max_blocks):
  """The loss arithmetic inside the per-range loop: n_ranges times, and not at all for an empty table."""
  scal = {k: buf[lay[k]] for k in ('loss_acc', 'loss_mean')}
  R.reference(buf, lay, ranges, mode, inv_k)
  for k, v in scal.items():
    buf[lay[k]] = v
  for _ in ranges:
    R.loss_arithmetic(buf, lay, mode, inv_k)


def _acc_written_in_last(buf, lay, ranges, mode, inv_k, max_blocks):
  R.reference(buf, lay, ranges, mode, inv_k)
  if mode == R.LAST:
    for o, l in ranges:
      buf[lay['acc'] + o:lay['acc'] + o + l] = buf[lay['g'] + o:lay['g'] + o + l]


def _writes_into_gaps(buf, lay, ranges, mode, inv_k, max_blocks):
  """One span from the first range's start to the last range's end."""
  if ranges:
    lo, hi = ranges[0][0], max(o + l for o, l in ranges)
    R.reference(buf, lay, [(lo, hi - lo)], mode, inv_k)
  else:
    R.reference(buf, lay, ranges, mode, inv_k)


def _pads_ranges_to_quads(buf, lay, ranges, mode, inv_k, max_blocks):
  """Moves whole 16-byte quads: up to three elements behind a range's end."""
  R.reference(buf, lay, [(o, -(-l // 4) * 4) for o, l in ranges], mode, inv_k)


def _fused_loss_mean(buf, lay, ranges, mode, inv_k, max_blocks):
  la, l = A.floats(buf[lay['loss_acc']:lay['loss_acc'] + 1])[0], A.floats(buf[lay['loss']:lay['loss'] + 1])[0]
  R.reference(buf, lay, ranges, mode, inv_k)
  if mode == R.LAST:
    p = np.float64(R.F32(l * R.F32(inv_k)))
    buf[lay['loss_mean']] = A.bits(R.F32(np.float64(la) * np.float64(R.F32(inv_k)) + p))[0]


def _first_adds(buf, lay, ranges, mode, inv_k, max_blocks):
  R.reference(buf, lay, ranges, R.ADD if mode == R.FIRST else mode, inv_k)


MUTANTS = {
    'range_end_one_past': _end_one_past,
    'range_end_one_short': _end_one_short,
    'second_range_skipped': _second_range_skipped,
    'tail_dropped': _tail_dropped,
    'loss_arithmetic_once_per_range': _loss_per_range,
    'acc_written_in_last': _acc_written_in_last,
    'write_into_a_gap': _writes_into_gaps,
    'ranges_padded_to_whole_quads': _pads_ranges_to_quads,
    'fused_multiply_add_in_the_loss_mean': _fused_loss_mean,
    'first_adds_into_stale_acc': _first_adds,
}


def _complaints(impl):
  out = []
  for c in CASES:
    for mode in R.MODES:
      out += [(c['name'], mode, m) for m in R.check_stage(impl, c, mode)]
    out += [(c['name'], 'chain', m) for m in R.check_chain(impl, c)]
  return out


def test_the_reference_passes_its_own_cases():
  assert _complaints(R.reference) == []


@pytest.mark.parametrize('name', sorted(MUTANTS))
def test_mutant_is_rejected(name):
  assert _complaints(MUTANTS[name]), 'the case set does not reject %s' % name


def test_each_mutant_is_caught_where_expected():
  kinds = lambda name: {(c, m.split(':')[0]) for c, _, m in _complaints(MUTANTS[name])}
  hit = lambda name, kind: {c for c, k in kinds(name) if k == kind}
  assert 'one_5_inside' in hit('range_end_one_past', 'untouched') and 'one_5_to_n' in hit('range_end_one_past', 'untouched')
  assert 'one_1_inside' in hit('range_end_one_short', 'value')
  assert {'two_touching', 'two_gap4', 'eight_touching'} <= hit('second_range_skipped', 'value')
  assert {'one_1_inside', 'one_3_to_n', 'one_4097_inside'} <= hit('tail_dropped', 'value')
  assert not hit('tail_dropped', 'untouched') and 'one_4096_inside' not in hit('tail_dropped', 'value')
  assert {'empty_table_with_loss', 'two_empty', 'eight_gap4'} <= hit('loss_arithmetic_once_per_range', 'value')
  assert 'head_and_tail' in hit('acc_written_in_last', 'untouched')
  assert {'two_gap4', 'eight_gap4', 'head_and_tail'} <= hit('write_into_a_gap', 'untouched')
  assert 'two_touching' not in hit('write_into_a_gap', 'untouched')
  assert {'one_1_inside', 'one_4095_to_n', 'two_gap4'} <= hit('ranges_padded_to_whole_quads', 'untouched')
  assert {c for c, _ in kinds('fused_multiply_add_in_the_loss_mean')} == {c['name'] for c in CASES}
  assert 'specials_nan' in hit('first_adds_into_stale_acc', 'value')
