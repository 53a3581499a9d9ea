"""CPU checks of the training summaries: the NumPy reference (tests/summary_ref.py) against hand-computed cases, the power of
the GPU case set (every mutant kernel is rejected by at least one case) and the host side of rigl_amd.summaries -- the record
parser, the dict builder and the ring ledger -- which is pure arithmetic."""
import json
import math

import numpy as np
import pytest

import summary_ref as R
from rigl_amd import summaries as S

F32 = np.float32


def _entry(w, g, mask=None, wd=0.0, apply_mask=1, pad=(7.0, 11.0)):
  n = len(w)
  bits = None
  if mask is not None:
    padded = np.ones((n + 31) // 32 * 32 + 32, np.uint8)
    padded[:n] = mask
    bits = np.packbits(padded, bitorder='little').view(np.uint32).copy()
  return {'n': n, 'w_buf': np.concatenate([np.asarray(w, F32), [F32(pad[0])]]),
          'g_buf': np.concatenate([np.asarray(g, F32), [F32(pad[1])]]), 'bits': bits, 'weight_decay': wd, 'apply_mask': apply_mask}


def test_reference_on_hand_computed_cases():
  # mask 1,0,1; grad_scale 0.5; no decay: gq = (1, 0, -3)
  out = R.entry_sums(_entry([1.0, -2.0, 0.5], [2.0, 100.0, -6.0], mask=[1, 0, 1]), 0.5)
  assert out == {'sumsq_g': 10.0, 'sumsq_w': 5.25, 'l1_w': 3.5, 'nz_w': 3, 'mask_ones': 2, 'nonfinite_g': 0}
  # decay 0.5 reaches masked-off weights: gq = (1 + 0.5, 0 - 1, -3 + 0.25)
  out = R.entry_sums(_entry([1.0, -2.0, 0.5], [2.0, 100.0, -6.0], mask=[1, 0, 1], wd=0.5), 0.5)
  assert out['sumsq_g'] == 1.5 ** 2 + 1.0 + 2.75 ** 2
  # apply_mask = 0: the dense gradient, the bitmap still counted
  out = R.entry_sums(_entry([1.0, -2.0, 0.5], [2.0, 100.0, -6.0], mask=[1, 0, 1], apply_mask=0), 0.5)
  assert out['sumsq_g'] == 1.0 + 2500.0 + 9.0 and out['mask_ones'] == 2
  # no bitmap: all ones, mask_ones = n; zeros of either sign are zero, subnormals are not
  out = R.entry_sums(_entry([0.0, -0.0, 1e-42, 3.0], [0.0, 0.0, 0.0, 4.0]), 1.0)
  assert out['nz_w'] == 2 and out['mask_ones'] == 4 and out['sumsq_g'] == 16.0
  assert out['l1_w'] == 3.0 + float(F32(1e-42)) and out['sumsq_w'] == 9.0 + float(F32(1e-42)) ** 2
  # every rounding point: f32(0.1f * 3) + f32(0.3f * 7), each product and the sum rounded to fp32
  gq = F32(F32(F32(0.1) * F32(3.0)) + F32(F32(0.3) * F32(7.0)))
  out = R.entry_sums(_entry([7.0], [3.0], wd=0.3), 0.1)
  assert out['sumsq_g'] == float(gq) * float(gq)
  # a non-finite gradient: counted and propagated where the mask is on, a zero where it is off
  out = R.entry_sums(_entry([1.0, 1.0], [np.inf, 2.0], mask=[1, 1]), 1.0)
  assert out['sumsq_g'] == math.inf and out['nonfinite_g'] == 1
  out = R.entry_sums(_entry([1.0, 1.0], [np.nan, 2.0], mask=[1, 1]), 1.0)
  assert math.isnan(out['sumsq_g']) and out['nonfinite_g'] == 1
  out = R.entry_sums(_entry([1.0, 1.0], [np.inf, 2.0], mask=[0, 1]), 1.0)
  assert out['sumsq_g'] == 4.0 and out['nonfinite_g'] == 0
  # the empty entry
  out = R.entry_sums(_entry([], []), 1.0)
  assert out == {'sumsq_g': 0.0, 'sumsq_w': 0.0, 'l1_w': 0.0, 'nz_w': 0, 'mask_ones': 0, 'nonfinite_g': 0}


def test_the_sum_is_exactly_rounded_and_the_bound_holds_for_any_fp64_order():
  rs = np.random.RandomState(0)
  x = rs.randn(20000).astype(F32)
  e = _entry(x, x)
  ref = R.entry_sums(e, 1.0)['sumsq_w']
  from fractions import Fraction
  exact = sum(Fraction(float(v)) ** 2 for v in x)
  assert ref == float(exact)                                        # Fraction -> float rounds to nearest
  sq = x.astype(np.float64) ** 2
  for order in (sq, sq[::-1], np.sort(sq), np.sort(sq)[::-1]):
    acc = 0.0
    for v in order:
      acc += v
    assert abs(acc - ref) <= R.bound(len(x), ref)
  assert abs(float(np.sum(sq)) - ref) <= R.bound(len(x), ref)       # numpy's pairwise order


@pytest.fixture(scope='module')
def case_set():
  tabs = R.tables()
  return [(t, R.table_sums(t)[0]) for t in tabs]


def test_case_set_covers_what_the_issue_lists(case_set):
  tabs = [t for t, _ in case_set]
  sizes = {e['n'] for t in tabs for e in t['entries']}
  assert set(R.EDGE_SIZES) <= sizes and 0 in sizes
  assert any(len(t['entries']) >= 300 for t in tabs)
  assert sum(t['W'].size for t in tabs) <= 1 << 20
  for t in tabs:
    for e in t['entries']:
      assert e['offset'] % 4 == 0                                   # 16-byte aligned slices


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_every_mutant_is_rejected_by_the_case_set(case_set, mutant):
  hits = []
  for t, ref in case_set:
    got = R.table_sums(t, mutant)[0]
    if R.differs(got, ref, [e['n'] for e in t['entries']]):
      hits.append(t['name'])
  assert hits, 'no case of the GPU set tells the mutant "%s" from the reference' % mutant


def test_the_reference_passes_its_own_check(case_set):
  for t, ref in case_set:
    assert not R.differs(ref, ref, [e['n'] for e in t['entries']])


# ---- the host side of rigl_amd.summaries -----------------------------------------------------------------------------------
def _slot(step, loss, lr, groups):
  """A ring slot as the kernel lays it out: groups = [(3 floats, 3 ints)] totals first."""
  n = len(groups) - 1
  buf = np.zeros(S.slot_bytes(n), np.uint8)
  buf[:8] = np.array([step, n], np.int32).view(np.uint8)
  buf[8:16] = np.array([loss, lr], np.float32).view(np.uint8)
  for k, (f, c) in enumerate(groups):
    o = S.HEADER_BYTES + k * S.GROUP_BYTES
    buf[o:o + 24] = np.array(f, np.float64).view(np.uint8)
    buf[o + 24:o + 48] = np.array(c, np.int64).view(np.uint8)
  return buf


LAYOUT = [
    {'name': 'conv1/weights:0', 'n': 100, 'weight_decay': 1e-4, 'mask': 'conv1/mask:0'},
    {'name': 'conv2/weights:0', 'n': 300, 'weight_decay': 5e-4, 'mask': 'conv2/mask:0'},
    {'name': 'fc/weights:0', 'n': 50, 'weight_decay': 1e-4, 'mask': None},
    {'name': 'bn/gamma:0', 'n': 8, 'weight_decay': 0.0, 'mask': None},
]
GROUPS = [((9.0, 16.0, 40.0), (200, 138, 0)),            # totals
          ((1.0, 4.0, 10.0), (20, 20, 0)), ((3.0, 6.0, 20.0), (122, 60, 0)), ((4.0, 5.0, 8.0), (50, 50, 0)),
          ((1.0, 1.0, 2.0), (8, 8, 0))]


def test_slot_bytes_and_parse():
  assert S.slot_bytes(0) == 64 and S.slot_bytes(1) == 128 and S.slot_bytes(4) == 256 and S.slot_bytes(5) == 320
  rec = S.parse_slot(_slot(7, 2.5, 0.125, GROUPS), 4)
  assert rec['step'] == 7 and rec['n_entries'] == 4 and rec['loss'] == 2.5 and rec['learning_rate'] == 0.125
  assert rec['totals'] == {'sumsq_g': 9.0, 'sumsq_w': 16.0, 'l1_w': 40.0, 'nz_w': 200, 'mask_ones': 138, 'nonfinite_g': 0}
  assert rec['entries']['sumsq_w'].tolist() == [4.0, 6.0, 5.0, 1.0]
  assert rec['entries']['mask_ones'].tolist() == [20, 60, 50, 8]


def test_dict_builder_names_and_arithmetic():
  from rigl_amd import sparse_utils
  rec = S.parse_slot(_slot(7, 2.5, 0.125, GROUPS), 4)
  d = S.make_record(rec, LAYOUT, steps_per_epoch=2.0, drop_fraction=lambda s: 0.25 + s)
  reg = 1e-4 * 4.0 / 2.0 + 5e-4 * 6.0 / 2.0 + 1e-4 * 5.0 / 2.0
  assert d['global_step'] == 7 and d['cross_loss'] == 2.5 and d['learning_rate'] == 0.125
  assert d['reg_loss'] == reg and d['loss'] == 2.5 + reg
  assert d['current_epoch'] == 3.5 and d['drop_fraction'] == 7.25
  assert d['grad_norm'] == 3.0 and d['var_norm'] == 4.0 and d['grad_nonfinite'] == 0
  assert d['fw_nz_weight'] == 20 and d['fw_nz_mask'] == 20 and d['fw_l1_weight'] == 10.0

  class M:                                                          # what calculate_sparsity reads of a mask variable
    def __init__(self, numel, ones):
      self.numel, self._ones = numel, ones

    def sum(self):
      return self._ones
  assert d['global_sparsity'] == sparse_utils.calculate_sparsity([M(100, 20), M(300, 60)])
  assert d['pruning/conv1/mask/sparsity'] == float(F32(1) - F32(F32(20) / F32(100)))
  assert d['pruning/conv2/mask/sparsity'] == float(F32(1) - F32(F32(60) / F32(300)))
  assert set(d) == {'global_step', 'loss', 'cross_loss', 'reg_loss', 'learning_rate', 'current_epoch', 'drop_fraction',
                    'grad_norm', 'var_norm', 'grad_nonfinite', 'fw_nz_weight', 'fw_nz_mask', 'fw_l1_weight', 'global_sparsity',
                    'pruning/conv1/mask/sparsity', 'pruning/conv2/mask/sparsity'}
  # optional keys are absent, not None; per-variable sums on request
  d2 = S.make_record(rec, LAYOUT, per_variable=True)
  assert 'current_epoch' not in d2 and 'drop_fraction' not in d2
  assert d2['per_variable']['fc/weights:0'] == {'sumsq_g': 4.0, 'sumsq_w': 5.0, 'l1_w': 8.0, 'nz_w': 50, 'mask_ones': 50,
                                                'nonfinite_g': 0}
  with pytest.raises(ValueError):
    S.make_record(rec, LAYOUT[:3])


def test_a_blown_up_step_shows_inf_or_nan():
  g = [((math.inf, math.nan, 1.0), (0, 0, 3))] + GROUPS[1:]
  d = S.make_record(S.parse_slot(_slot(0, math.nan, 0.1, g), 4), LAYOUT)
  assert d['grad_norm'] == math.inf and math.isnan(d['var_norm']) and d['grad_nonfinite'] == 3 and math.isnan(d['loss'])


def test_ring_ledger_wrap_order_and_dropped():
  L = S.RingLedger(4)
  for s in range(11):
    L.wrote(s)
  live, dropped = L.take()
  assert [s for _, s in live] == [7, 8, 9, 10] and [slot for slot, _ in live] == [3, 0, 1, 2] and dropped == 7
  assert L.take() == ([], 0)
  # a capture's write is undone, also where it displaced a record
  for s in range(11, 15):
    L.wrote(s)
  L.wrote(15)
  L.undo()
  live, dropped = L.take()
  assert sorted(s for _, s in live) == [11, 12, 13, 14] and dropped == 0
  L.wrote(3)
  L.undo()
  assert L.take() == ([], 0)
  with pytest.raises(RuntimeError):
    L.undo()
  # an assigned step lands in its own slot; negative (wrapped) steps map as the kernel's non-negative remainder
  L.wrote(5)
  L.wrote(40)
  L.wrote(41)
  assert L.take() == ([(0, 40), (1, 41)], 1) and L.slot_of(-1) == 3 and L.slot_of(2 ** 31) == 0
  with pytest.raises(ValueError):
    S.RingLedger(0)


def test_write_jsonl(tmp_path):
  p = tmp_path / 's.jsonl'
  S.write_jsonl(str(p), [{'global_step': 1, 'loss': 0.5, 'grad_norm': math.inf}, {'global_step': 2, 'loss': math.nan}])
  S.write_jsonl(str(p), [{'global_step': 3, 'loss': np.float32(0.25), 'n': np.int64(4)}])
  rows = [json.loads(l) for l in open(str(p))]
  assert rows == [{'global_step': 1, 'loss': 0.5, 'grad_norm': 'inf'}, {'global_step': 2, 'loss': 'nan'},
                  {'global_step': 3, 'loss': 0.25, 'n': 4}]


def test_reference_module_path_alias():
  from rigl.imagenet_resnet import utils
  assert utils.mask_summaries is S.mask_summaries


def test_the_abi_constants_agree_with_the_header():
  import os
  import re
  from rigl_amd import _lib
  txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rigl_hip.h')).read()
  assert int(re.search(r'#define RIGL_SUMMARY_CHUNK (\d+)', txt).group(1)) == _lib.SUMMARY_CHUNK == R.CHUNK
  assert {'rigl_summary_step', 'rigl_summary_slot_bytes', 'rigl_summary_workspace_bytes'} <= set(_lib.SIGNATURES)
  lib = _lib.load()
  for n in (0, 1, 4, 5, 300):
    assert lib.rigl_summary_slot_bytes(n) == S.slot_bytes(n)
  # refusals that need no device: nothing is launched for any of them
  step = 4096
  assert lib.rigl_summary_step(None, 1, 1.0, None, None, 0.1, step, 4096, 4, None, 0, 0, None) == _lib.RIGL_EINVAL
  e = (_lib.SummaryEntry * 1)()
  e[0].n, e[0].w, e[0].g = 8, 4096, 8192
  need = lib.rigl_summary_workspace_bytes(e, 1)
  assert need == 256 + 256
  assert lib.rigl_summary_step(e, 1, 1.0, None, None, 0.1, step, 4096, 0, 256, need, 0, None) == _lib.RIGL_EINVAL
  assert lib.rigl_summary_step(e, 1, 1.0, None, None, 0.1, step, 4096, 4, None, need, 0, None) == _lib.RIGL_EWORKSPACE
  assert lib.rigl_summary_step(e, 1, 1.0, None, None, 0.1, step, 4096, 4, 256, need - 1, 0, None) == _lib.RIGL_EWORKSPACE
  e[0].w = 4100
  assert lib.rigl_summary_step(e, 1, 1.0, None, None, 0.1, step, 4096, 4, 256, need, 0, None) == _lib.RIGL_EINVAL
  assert b'16-byte' in lib.rigl_last_error()
  e[0].w, e[0].mask_bits = 4096, 4098
  assert lib.rigl_summary_step(e, 1, 1.0, None, None, 0.1, step, 4096, 4, 256, need, 0, None) == _lib.RIGL_EINVAL
  assert b'mask_bits' in lib.rigl_last_error()
