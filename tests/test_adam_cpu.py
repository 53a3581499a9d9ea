"""Adam as an inner optimizer, host side: the fp32 restatement of ApplyAdam
(tests/adam_ref.py) against the reference-executed fixtures
(tests/golden/adam_cases.npz, written by make_golden_adam.py), the beta-power
recurrence, the slot surface of train.AdamOptimizer and the two-slot limit of
the fused mask update."""
import ctypes
import os

import numpy as np
import pytest

import adam_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'adam_cases.npz')
F32 = np.float32


def _traj(tag):
  t = np.load(GOLDEN)
  p = 'traj_%s__' % tag
  return {k[len(p):]: t[k] for k in t.files if k.startswith(p)}


@pytest.mark.parametrize('tag', ['acc0', 'acc05'])
def test_restatement_reproduces_every_adam_transition(tag):
  """Every ordinary step of the reference run is one ApplyAdam of the restatement (bit-exact); every mask-update
  step leaves the slots of kept connections alone and resets both slots of grown ones to dense * acc_scale."""
  T = _traj(tag)
  W, M, GS, BP = T['w'], T['mask'], T['gs'], T['bp']
  n_inp, n_out = W.shape[1:]
  m = np.zeros((n_inp, n_out), F32)
  v = np.zeros((n_inp, n_out), F32)
  bp = np.array([0.9, 0.999], F32)
  n_apply = n_update = 0
  for i in range(len(BP)):
    gs = int(GS[i])
    dense = np.broadcast_to((np.arange(n_out, dtype=F32) * F32(gs)).astype(F32), (n_inp, n_out)).astype(F32)
    if GS[i + 1] == gs + 1:                 # ordinary step: the inner optimizer applied
      g = R.masked_grad(dense, M[i], W[i])
      w, m, v = R.adam_apply(W[i], m, v, g, T['lr'], bp)
      bp = R.advance(bp)
      assert np.array_equal(M[i + 1], M[i]), 'step %d' % i
      n_apply += 1
    else:                                   # mask update: no apply, the step and the powers stay
      assert GS[i + 1] == gs
      grown = (M[i + 1] > 0) & (M[i] == 0)
      reset = (dense * F32(T['acc_scale'])).astype(F32)
      w = np.where(grown, F32(0), W[i]).astype(F32)
      m = np.where(grown, reset, m).astype(F32)
      v = np.where(grown, reset, v).astype(F32)
      n_update += 1
    assert R.same_bits(w, W[i + 1]), 'w, step %d' % i
    assert R.same_bits(m, T['m'][i]), 'm, step %d' % i
    assert R.same_bits(v, T['v'][i]), 'v, step %d' % i
    assert np.array_equal(bp.view(np.uint32), BP[i].view(np.uint32)), 'beta powers, step %d' % i
  assert n_apply >= 15 and n_update >= 4


def test_beta_powers_are_iterated_fp32_products():
  T = _traj('acc0')
  applies = np.diff(T['gs'])          # 1 where the inner optimizer applied
  b1, b2 = F32(0.9), F32(0.999)
  p1, p2 = b1, b2
  for i, a in enumerate(applies):
    if a:
      p1, p2 = F32(p1 * b1), F32(p2 * b2)
    assert T['bp'][i][0] == p1 and T['bp'][i][1] == p2


def test_single_update_cases_reset_both_slots():
  """The fixtures of one mask update: both slots of every new connection carry the reset value, every other slot
  entry is untouched (SET: zeros; RigL: dense_grad * initial_acc_scale; reinit_when_same: mask2, not mask1 | mask2)."""
  t = np.load(GOLDEN)
  tags = sorted({k.split('__')[0] for k in t.files if k.startswith('single_')})
  assert len(tags) == 6
  for tag in tags:
    c = {k.split('__')[1]: t[k] for k in t.files if k.startswith(tag + '__')}
    changed = (c['new_m'] != c['m']) | (c['new_v'] != c['v'])
    reset = (c['dense_grad'] * c['acc_scale']).astype(F32) if c['momreset'] else np.zeros_like(c['w'])
    assert np.array_equal(c['new_m'][changed], reset[changed]), tag
    assert np.array_equal(c['new_v'][changed], reset[changed]), tag
    assert changed.sum() > 0 and not (changed & (c['new_mask'] == 0)).any(), tag
    if c['reinit']:
      kept_regrown = (c['mask'] > 0) & (c['new_mask'] > 0) & changed
      assert kept_regrown.any(), tag        # reinit_when_same touched kept connections that were re-grown


def test_adam_slot_surface():
  from rigl_amd import train
  opt = train.AdamOptimizer()
  assert opt.get_slot_names() == ['m', 'v']
  assert (opt._lr, opt._beta1, opt._beta2, opt._epsilon) == (0.001, 0.9, 0.999, 1e-8)
  with pytest.raises(KeyError):
    opt.get_slot(object(), 'momentum')


def test_more_than_two_slots_raise_on_the_fused_path():
  from rigl_amd import sparse_optimizers as SO
  from rigl_amd import train

  class ThreeSlots(train.GradientDescentOptimizer):

    def get_slot_names(self):
      return ['a', 'b', 'c']

  class Layer:
    weights = None

  for cls in (SO.SparseRigLOptimizer, SO.SparseSETOptimizer):
    opt = cls(ThreeSlots(0.1), 0, 10, 1)
    with pytest.raises(NotImplementedError):
      opt._slots_of(Layer())


def test_second_slot_reset_needs_the_dense_gradient():
  """rigl_prune_regrow_slots validates a second slot like momentum: a RigL reset with acc_scale != 0 needs dense_grad
  (argument checks only: the call returns before anything is enqueued)."""
  from rigl_amd import _lib
  lib = _lib.load()
  lay = _lib.PruneRegrowLayer(64, 1, None, 1, None, None, 1, 1, None)   # w, mask_bits, scores: never dereferenced
  prm = _lib.PruneRegrowParams(0.1, 0, 1.0, _lib.MOMRESET_GRAD, 0.5, 0)
  m2 = (ctypes.c_void_p * 1)(1)
  assert lib.rigl_prune_regrow_slots(ctypes.byref(lay), m2, 1, ctypes.byref(prm), None, None, 0, None) == _lib.RIGL_EINVAL
  assert b'dense_grad' in lib.rigl_last_error()
  assert lib.rigl_masked_adam(8, None, None, None, None, None, None, 0.1, 0.9, 0.999, 1e-8, 0.0, 1.0, None,
                              None) == _lib.RIGL_EINVAL
  assert lib.rigl_adam_advance(None, 0.9, 0.999, None) == _lib.RIGL_EINVAL
