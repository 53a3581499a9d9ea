"""bn3's backward apply on the 1x1 backward's operand load, in the training step: one ResNet-50 step at batch 8 with knob
"bn_bwd_on_load" on against the same step with it off.  The loss, the whole gradient arena, the weights and momentum the
update leaves and every moving mean and variance must be bit-identical; with the knob on the two identity blocks of group 1
must really take the fused backward (counted), with it off none.  Knobs "bwd1x1" = 2 and "rs_masked_addend" = 2 in both arms:
at batch 8 the 56x56 layers have 25 088 rows, below the default rules' row count for the single-pass 1x1 backward and for the
unmasked hand-over of the shortcut gradient.

The conv node must refuse a gradient it cannot trust: a holder whose contents were swapped, or emptied, after the batch norm
filled it makes the backward raise instead of running the kernel on the wrong tensor.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BATCH = 8


def _build():
  from rigl_amd import sparse_utils, train, variables as V
  from rigl_amd.workloads import nn as gnn, resnet50
  g = V.reset_default_graph(DEV)
  model = resnet50.ResNet50(g, seed=0)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
  images, labels = resnet50.synthetic_batch(BATCH, DEV, seed=1234)
  opt = train.MomentumOptimizer(0.1, 0.9, use_nesterov=True, graph=g)
  bns = [mod for mod in g.modules.values() if isinstance(mod, gnn.BatchNorm)]
  return g, model, images, labels, opt, bns


def _step(knob, monkeypatch):
  from rigl_amd import ops
  calls = []
  real = ops.conv_bwd_bnapply
  monkeypatch.setattr(ops, 'conv_bwd_bnapply', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
  ops.tune_set('bwd1x1', 2)
  ops.tune_set('rs_masked_addend', 2)
  ops.tune_set('bn_bwd_on_load', knob)
  try:
    g, model, images, labels, opt, bns = _build()
    loss = model.loss(images, labels, label_smoothing=0.1)
    opt.minimize(loss, g.get_or_create_global_step())
    torch.cuda.synchronize()
    return dict(loss=loss.detach().float().cpu().numpy().copy(), G=g.G.cpu().numpy().copy(), W=g.W.cpu().numpy().copy(),
                A=opt._slot.cpu().numpy().copy(),  # pylint: disable=protected-access
                mm=[b.moving_mean.cpu().numpy().copy() for b in bns], mv=[b.moving_variance.cpu().numpy().copy() for b in bns],
                calls=len(calls))
  finally:
    ops.tune_unset('bwd1x1')
    ops.tune_unset('rs_masked_addend')
    ops.tune_unset('bn_bwd_on_load')


def test_step_is_bit_identical_with_the_knob_on_and_off(monkeypatch):
  off = _step(0, monkeypatch)
  on = _step(1, monkeypatch)
  assert off['calls'] == 0, 'knob 0 must be the former path'
  assert on['calls'] == 2, 'the two identity blocks of group 1 take the fused backward, got %d' % on['calls']
  assert np.isfinite(on['loss']).all()
  np.testing.assert_array_equal(on['loss'].view(np.uint32), off['loss'].view(np.uint32))
  np.testing.assert_array_equal(on['G'].view(np.uint32), off['G'].view(np.uint32))
  np.testing.assert_array_equal(on['W'].view(np.uint32), off['W'].view(np.uint32))
  np.testing.assert_array_equal(on['A'].view(np.uint32), off['A'].view(np.uint32))
  assert len(on['mm']) == len(off['mm']) == 53
  for a, b in zip(on['mm'] + on['mv'], off['mm'] + off['mv']):
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize('how', ('swapped', 'emptied', 'disarmed'))
def test_conv_node_raises_on_a_tampered_holder(how, monkeypatch):
  from rigl_amd import ops, pruning_layers as PL
  real = PL.BnApplyHolder.fill
  if how == 'swapped':       # another tensor than the gradient the batch norm returns
    monkeypatch.setattr(PL.BnApplyHolder, 'fill', lambda self, dout, *a: real(self, dout.clone(), *a))
  elif how == 'emptied':     # the batch norm skipped its apply pass but left nothing
    monkeypatch.setattr(PL.BnApplyHolder, 'fill', lambda self, *a: None)
  else:                      # the forward-time decision flipped behind the batch norm's back
    def fill(self, *a):
      real(self, *a)
      self.armed = False
    monkeypatch.setattr(PL.BnApplyHolder, 'fill', fill)
  ops.tune_set('bwd1x1', 2)
  ops.tune_set('rs_masked_addend', 2)
  ops.tune_set('bn_bwd_on_load', 1)
  try:
    _, model, images, labels, _, _ = _build()
    loss = model.loss(images, labels, label_smoothing=0.1)
    with pytest.raises(RuntimeError, match='bn_bwd_on_load'):
      loss.backward()
    torch.cuda.synchronize()
  finally:
    ops.tune_unset('bwd1x1')
    ops.tune_unset('rs_masked_addend')
    ops.tune_unset('bn_bwd_on_load')
