"""The shortcut gradient's hand-over between relu(bn3 + shortcut) and the block's first conv (pruning_layers.MaskedAddendHolder):
the batch norm returns the block-output gradient itself, UNMASKED, as the shortcut's and leaves the ReLU bits in the holder that
conv1's fork put on the alias; conv1's backward masks on the fly (rigl_masked_conv2d_bwd_masked) -- but only the very tensor that
was handed over.  Anything else must raise: added as it is, an unmasked gradient is a silently wrong dX.

One identity bottleneck built by hand at the 56x56 shape of ResNet-50's group 1 and batch 8 (25 088 rows: the masked form is
legal only with knob "rs_masked_addend" = 2): x [8, 56, 56, 256] -> conv1 1x1 256 -> 64 (fork) -> bn1 + ReLU -> 3x3 64 -> 64 ->
bn2 + ReLU -> 1x1 64 -> 256 -> relu(bn3 + alias), bn3's gamma 0.5.  Reference for the bits: the same backward with the masked
copy written (nn._LAZY_RES_GRAD False), the relu / add gradients of bottleneck_block_ through autodiff (resnet_model.py:497-501).
"""
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _backward(monkeypatch, lazy, second_reader=False):
  """One forward + backward of the block; returns the bits of x.grad and of the three weight gradients, and how many one-call
  backwards were given ``addend_bits``."""
  from rigl_amd import ops, pruning_layers as PL, variables as V
  from rigl_amd.workloads import nn as gnn
  monkeypatch.setattr(gnn, '_LAZY_RES_GRAD', bool(lazy))
  masked = []
  real = ops.conv_bwd
  monkeypatch.setattr(ops, 'conv_bwd', lambda *a, **k: (masked.append(1) if k.get('addend_bits') is not None else None,
                                                        real(*a, **k))[1])
  ops.tune_set('rs_masked_addend', 2)
  try:
    g = V.reset_default_graph(DEV)
    PL.set_init_seed(3)
    c1 = PL.MaskedConv2d(g, 'c1', 256, 64, (1, 1), (1, 1), 'SAME', 'threshold', 0.0)
    bn1 = gnn.BatchNorm(g, 'bn1', 64)
    c2 = PL.MaskedConv2d(g, 'c2', 64, 64, (3, 3), (1, 1), 'SAME', 'threshold', 0.0)
    bn2 = gnn.BatchNorm(g, 'bn2', 64)
    c3 = PL.MaskedConv2d(g, 'c3', 64, 256, (1, 1), (1, 1), 'SAME', 'threshold', 0.0)
    bn3 = gnn.BatchNorm(g, 'bn3', 256, init_zero=True)
    g.finalize()
    bn3.gamma.data.fill_(0.5)
    gen = torch.Generator(device=DEV).manual_seed(11)
    for l in (c1, c2, c3):                                 # random 50 % masks
      l.mask.assign((torch.rand(l.weights.shape, generator=gen, device=DEV) < 0.5).float())
    x = torch.randn(8, 56, 56, 256, generator=gen, device=DEV).to(torch.bfloat16).requires_grad_(True)
    gy = torch.randn(8, 56, 56, 256, generator=gen, device=DEV).to(torch.bfloat16)
    assert c1.takes_masked_addend(x), 'the block must be one whose first conv takes the unmasked shortcut gradient'
    y, alias = c1.fork(x, bn_stats=True)
    y = bn1(y, True, relu=True)
    y = bn2(c2(y, bn_stats=True), True, relu=True)
    out = bn3(c3(y, bn_stats=True), True, relu=True, residual=alias)
    if second_reader:                                      # autograd then SUMS the alias' two gradients into a new tensor
      torch.autograd.backward([out, alias.float().sum() * 0], [gy, None])
    else:
      out.backward(gy)
    torch.cuda.synchronize()
    return dict(dx=x.grad.view(torch.int16).clone(), dw=[l.weights.grad.view(torch.int32).clone() for l in (c1, c2, c3)],
                masked=len(masked))
  finally:
    ops.tune_unset('rs_masked_addend')


@pytest.fixture(scope='module')
def eager():
  """The block's gradients with the masked copy written (the hand-over switched off): computed once."""
  mp = pytest.MonkeyPatch()
  try:
    return _backward(mp, lazy=False)
  finally:
    mp.undo()


def test_handed_over_gradient_gives_the_bits_of_the_masked_copy(eager, monkeypatch):
  lazy = _backward(monkeypatch, lazy=True)
  assert lazy['masked'] == 1 and eager['masked'] == 0, (lazy['masked'], eager['masked'])
  assert bool(eager['dx'].any()), 'the reference gradient must not be all zeros'
  assert torch.equal(lazy['dx'], eager['dx']), 'x.grad differs with the masked copy skipped'
  for a, b, name in zip(lazy['dw'], eager['dw'], ('conv1', 'conv2', 'conv3')):
    assert torch.equal(a, b), '%s: weights.grad differs with the masked copy skipped' % name


@pytest.mark.parametrize('how', ('swapped', 'emptied', 'disarmed'))
def test_fork_refuses_a_tampered_holder(how, monkeypatch):
  from rigl_amd import pruning_layers as PL
  real = PL.MaskedAddendHolder.fill
  if how == 'swapped':       # another tensor than the gradient the batch norm returns
    monkeypatch.setattr(PL.MaskedAddendHolder, 'fill', lambda self, dy, *a: real(self, dy.clone(), *a))
  elif how == 'emptied':     # the batch norm skipped the masked copy but left nothing
    monkeypatch.setattr(PL.MaskedAddendHolder, 'fill', lambda self, *a: None)
  else:                      # the forward-time decision flipped behind the batch norm's back
    def fill(self, *a):
      real(self, *a)
      self.armed = False
    monkeypatch.setattr(PL.MaskedAddendHolder, 'fill', fill)
  with pytest.raises(RuntimeError, match='lazy_res_grad'):
    _backward(monkeypatch, lazy=True)
  torch.cuda.synchronize()


def test_fork_refuses_a_gradient_autograd_accumulated(monkeypatch):
  """The alias has a second reader: what reaches conv1 is the SUM of two gradients in a new tensor, which the ReLU bits do not
  belong to.  Added as it is, that sum would be a wrong dX that nothing reports: the backward must raise."""
  with pytest.raises(RuntimeError, match='lazy_res_grad'):
    _backward(monkeypatch, lazy=True, second_reader=True)
  torch.cuda.synchronize()
