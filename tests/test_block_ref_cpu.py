"""tests/block_ref.py (the float64 twins of the network blocks) checked on the CPU before a GPU test relies on them.

1. With ``rounding=False`` every output of every twin equals an independently written torch.nn MODULE formulation
   (Conv2d with its own padding argument, BatchNorm2d in training mode, MaxPool2d, AdaptiveAvgPool2d, Linear,
   CrossEntropyLoss) to 1e-12 relative in float64.  The twins pad by hand after resnet_model.fixed_padding and sum the
   loss by hand; the modules do neither.
2. The twin's max pool is the tie rule of tests/glue_ref.py (first maximum in row-major window order), on inputs full
   of ties.
3. Mutation sensitivity.  Each wiring fault below is seeded into a COPY of a twin (kept here, not in block_ref.py); the
   copy stands for a product with that fault, and at least one compared tensor must then leave block_ref.BOUND -- the
   bound tests/test_block_grad_gpu.py holds the product to -- so that the GPU test is known to fail on such a fault.
   The fp32-arithmetic twin must stay far inside the bound on the same operands (the comparison's noise floor).
"""
import pytest

torch = pytest.importorskip('torch')
import torch.nn as nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tests import block_ref as B  # noqa: E402
from tests import glue_ref  # noqa: E402

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def _sparse(g, *shape):
  fan_in = 1
  for s in shape[:-1]:
    fan_in *= s
  w = torch.randn(*shape, generator=g) * (2.0 / fan_in) ** 0.5
  return (w * (torch.rand(*shape, generator=g) < 0.2)).float()          # mask * W at 80 % sparsity


def _bn(g, c):
  return torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3


def _bottleneck_operands(seed, n, hw, cin, f, stride, proj):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(n, hw, hw, cin, generator=g).relu().to(torch.bfloat16)
  w = {'c1': _sparse(g, 1, 1, cin, f), 'c2': _sparse(g, 3, 3, f, f), 'c3': _sparse(g, 1, 1, f, 4 * f)}
  bn = {'bn1': _bn(g, f), 'bn2': _bn(g, f), 'bn3': _bn(g, 4 * f)}
  if proj:
    w['proj'] = _sparse(g, 1, 1, cin, 4 * f)
    bn['bn_proj'] = _bn(g, 4 * f)
  ho = (hw - 1) // stride + 1
  dy = torch.randn(n, ho, ho, 4 * f, generator=g).to(torch.bfloat16)
  return x, dy, w, bn


def _mobilenet_operands(seed, n, hw, c, f, stride):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(n, hw, hw, c, generator=g).relu().to(torch.bfloat16)
  w_dw = (torch.randn(3, 3, c, 1, generator=g) / 3.0).float()
  w_pw = _sparse(g, 1, 1, c, f)
  bn = {'bn_a': _bn(g, c), 'bn_b': _bn(g, f)}
  ho = (hw - 1) // stride + 1
  dy = torch.randn(n, ho, ho, f, generator=g).to(torch.bfloat16)
  return x, dy, w_dw, w_pw, bn


def _stem_operands(seed, n, hw, cout=16):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(n, hw, hw, 3, generator=g).to(torch.bfloat16)
  w = _sparse(g, 7, 7, 3, cout)
  bn = {'bn': _bn(g, cout)}
  ho = -(-((hw - 1) // 2 + 1) // 2)
  dy = torch.randn(n, ho, ho, cout, generator=g).to(torch.bfloat16)
  return x, dy, w, bn


def _head_operands(seed, n, hw, c, k):
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(n, hw, hw, c, generator=g).relu().to(torch.bfloat16)
  w = _sparse(g, c, k)
  bias = (torch.randn(k, generator=g) * 0.1).float()
  labels = torch.randint(0, k, (n,), generator=g)
  return x, labels, w, bias


def _close(got, ref, what, tol=1e-12):
  assert set(got) == set(ref), (sorted(got), sorted(ref))
  for k in ref:
    r = B.rel_l2(got[k], ref[k])
    assert r <= tol, (what, k, r)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the twins without rounding against torch.nn modules
# ---------------------------------------------------------------------------------------------------------------------
def _conv_module(w_hwio, stride=1, groups=1):
  kh, _, cin, cout = w_hwio.shape
  if groups > 1:                                             # depthwise [kh, kw, C, 1]
    cin = cout = groups
  m = nn.Conv2d(cin, cout, kh, stride=stride, padding=(kh - 1) // 2, bias=False, groups=groups).double()
  with torch.no_grad():
    m.weight.copy_(w_hwio.double().permute(3, 2, 0, 1) if groups == 1 else w_hwio.double().permute(2, 3, 0, 1))
  return m


def _bn_module(gamma_beta):
  gamma, beta = gamma_beta
  m = nn.BatchNorm2d(gamma.numel(), eps=1e-5, momentum=0.1).double().train()
  with torch.no_grad():
    m.weight.copy_(gamma.double())
    m.bias.copy_(beta.double())
  return m


class _BottleneckModule(nn.Module):
  """torchvision-style bottleneck (v1.5: the stride on the 3x3): Conv2d(k, stride, padding=(k - 1) // 2) IS fixed padding."""

  def __init__(self, w, bn, stride):
    super().__init__()
    self.c1, self.c2, self.c3 = _conv_module(w['c1']), _conv_module(w['c2'], stride), _conv_module(w['c3'])
    self.bn1, self.bn2, self.bn3 = _bn_module(bn['bn1']), _bn_module(bn['bn2']), _bn_module(bn['bn3'])
    self.down = nn.Sequential(_conv_module(w['proj'], stride), _bn_module(bn['bn_proj'])) if 'proj' in w else None

  def forward(self, x):
    idt = x if self.down is None else self.down(x)
    h = torch.relu(self.bn1(self.c1(x)))
    h = torch.relu(self.bn2(self.c2(h)))
    return torch.relu(self.bn3(self.c3(h)) + idt)


def _module_grads(out, x, convs, bns):
  if x is not None:
    out['dx'] = x.grad.permute(0, 2, 3, 1)
  for k, m in convs.items():
    out['dw_' + k] = m.weight.grad.permute(2, 3, 1, 0)
  for k, m in bns.items():
    out['dgamma_' + k], out['dbeta_' + k] = m.weight.grad, m.bias.grad
  return out


@pytest.mark.parametrize('hw,stride,proj', [(8, 1, False), (8, 1, True), (8, 2, True), (9, 2, True)])
def test_bottleneck_twin_equals_the_module_formulation(hw, stride, proj):
  x, dy, w, bn = _bottleneck_operands(1, 2, hw, 32 if proj else 64, 16, stride, proj)
  got = B.bottleneck(x, dy, w, bn, stride=stride, rounding=False)
  m = _BottleneckModule(w, bn, stride)
  xm = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
  y = m(xm)
  y.backward(dy.double().permute(0, 3, 1, 2))
  convs = {'c1': m.c1, 'c2': m.c2, 'c3': m.c3}
  bns = {'bn1': m.bn1, 'bn2': m.bn2, 'bn3': m.bn3}
  if proj:
    convs['proj'], bns['bn_proj'] = m.down[0], m.down[1]
  _close(got, _module_grads({'y': y.detach().permute(0, 2, 3, 1)}, xm, convs, bns), 'bottleneck')


@pytest.mark.parametrize('hw,stride', [(8, 1), (8, 2), (7, 2)])
def test_mobilenet_block_twin_equals_the_module_formulation(hw, stride):
  x, dy, w_dw, w_pw, bn = _mobilenet_operands(2, 2, hw, 16, 24, stride)
  got = B.mobilenet_block(x, dy, w_dw, w_pw, bn, stride=stride, rounding=False)
  dw = _conv_module(w_dw, stride, groups=16)
  pw, bn_a, bn_b = _conv_module(w_pw), _bn_module(bn['bn_a']), _bn_module(bn['bn_b'])
  xm = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
  y = torch.relu(bn_b(pw(torch.relu(bn_a(dw(xm))))))
  y.backward(dy.double().permute(0, 3, 1, 2))
  ref = _module_grads({'y': y.detach().permute(0, 2, 3, 1)}, xm, {'pw': pw}, {'bn_a': bn_a, 'bn_b': bn_b})
  ref['dw_dw'] = dw.weight.grad.permute(2, 3, 0, 1)
  _close(got, ref, 'mobilenet block')


def test_stem_twin_equals_the_module_formulation():
  """Even sizes: tf 'SAME' pooling pads only behind, which is MaxPool2d(3, 2, ceil_mode=True) without padding."""
  x, dy, w, bn = _stem_operands(3, 2, 24)
  got = B.resnet_stem(x, dy, w, bn, rounding=False)
  conv, bnm, pool = _conv_module(w, 2), _bn_module(bn['bn']), nn.MaxPool2d(3, 2, padding=0, ceil_mode=True)
  y = pool(torch.relu(bnm(conv(x.double().permute(0, 3, 1, 2)))))
  y.backward(dy.double().permute(0, 3, 1, 2))
  _close(got, _module_grads({'y': y.detach().permute(0, 2, 3, 1)}, None, {'stem': conv}, {'bn': bnm}), 'stem')


@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_head_twin_equals_the_module_formulation(eps):
  x, labels, w, bias = _head_operands(4, 5, 7, 24, 10)
  got = B.head(x, labels, w, bias, eps, rounding=False)
  fc = nn.Linear(24, 10).double()
  with torch.no_grad():
    fc.weight.copy_(w.double().t())
    fc.bias.copy_(bias.double())
  xm = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
  loss = nn.CrossEntropyLoss(label_smoothing=eps)(fc(nn.AdaptiveAvgPool2d(1)(xm).flatten(1)), labels)
  loss.backward()
  _close(got, {'y': loss.detach(), 'dx': xm.grad.permute(0, 2, 3, 1), 'dw_fc': fc.weight.grad.t(), 'dbias': fc.bias.grad}, 'head')


# ---------------------------------------------------------------------------------------------------------------------
# 2. the pool's tie rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['four_levels', 'normal', 'constant'])
@pytest.mark.parametrize('h,w', [(16, 16), (15, 13)])
def test_twin_max_pool_has_the_tie_rule_of_glue_ref(kind, h, w):
  d = glue_ref.same_pool_desc(2, h, w, 8, 3, 2)
  x = glue_ref.pool_input(kind, d, 5)
  dy = glue_ref.pool_dy(d, 5)
  y_ref, arg = glue_ref.maxpool_ref(x, d)
  dx_ref, _, _ = glue_ref.maxpool_bwd_ref(dy, arg, d)
  xm = x.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
  y = B.max_pool_3x3_s2_same(xm)
  y.backward(dy.double().permute(0, 3, 1, 2))
  assert torch.equal(y.detach().permute(0, 2, 3, 1), y_ref.double())
  assert torch.equal(xm.grad.permute(0, 2, 3, 1), dx_ref)


# ---------------------------------------------------------------------------------------------------------------------
# 3. mutation sensitivity
# ---------------------------------------------------------------------------------------------------------------------
class _AddReluUnmaskedShortcut(torch.autograd.Function):
  """relu(a + s) whose backward forgets the ReLU on the shortcut's side."""

  @staticmethod
  def forward(ctx, a, s):
    y = F.relu(a + s)
    ctx.save_for_backward(y)
    return y

  @staticmethod
  def backward(ctx, g):
    (y,) = ctx.saved_tensors
    return g * (y > 0), g


class _SubsampleOddGrad(torch.autograd.Function):
  """x[:, :, ::2, ::2] whose gradient lands on the pixels (2i + 1, 2j + 1)."""

  @staticmethod
  def forward(ctx, x):
    ctx.shape = x.shape
    return x[:, :, ::2, ::2]

  @staticmethod
  def backward(ctx, g):
    dx = g.new_zeros(ctx.shape)
    hh, ww = dx[:, :, 1::2, 1::2].shape[2:]
    dx[:, :, 1::2, 1::2] = g[:, :, :hh, :ww]
    return dx


class _GradTimes(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, k):
    ctx.k = k
    return x.view_as(x)

  @staticmethod
  def backward(ctx, g):
    return g * ctx.k, None


BOTTLENECK_FAULTS = ('shortcut_dropped', 'shortcut_after_conv1', 'shortcut_grad_unmasked', 'proj_grad_odd_pixels',
                     'same_padding_on_strided_3x3', 'bn3_dx_twice')


def _mutated_bottleneck(fault, x, dy, w, bn, stride=1, dtype=F64, rounding=True):
  """block_ref.bottleneck, copied, with one wiring fault seeded (``fault`` None: the copy itself, checked to be faithful)."""
  r = B.rounder(rounding)
  W = {k: B.conv_weight(v, dtype, rounding) for k, v in w.items()}
  Bn = {k: (B.leaf(g.to(dtype)), B.leaf(b.to(dtype))) for k, (g, b) in bn.items()}
  x0 = B.leaf(B.nchw(x, dtype))
  inputs = r(x0)
  h = r(B.conv2d_fixed_padding(r(inputs), W['c1'], 1))
  shortcut = inputs
  if 'proj' in W:
    src = r(inputs)
    if fault == 'shortcut_after_conv1':
      src = h                                                # (a group-1 first block: conv1's output has the input's channels)
    if fault == 'proj_grad_odd_pixels':
      assert stride == 2
      shortcut = r(F.conv2d(_SubsampleOddGrad.apply(src), W['proj']))
    else:
      shortcut = r(B.conv2d_fixed_padding(src, W['proj'], stride))
    shortcut = r(B.batch_norm(shortcut, *Bn['bn_proj']))
  h = r(F.relu(B.batch_norm(h, *Bn['bn1'])))
  if fault == 'same_padding_on_strided_3x3':
    assert stride == 2 and h.shape[2] % 2 == 0               # tf 'SAME' on an even size: nothing in front, one pixel behind
    h = r(F.conv2d(B.same_padding(h, 3, 2), W['c2'], stride=2))
  else:
    h = r(B.conv2d_fixed_padding(h, W['c2'], stride))
  h = r(F.relu(B.batch_norm(h, *Bn['bn2'])))
  h = r(B.conv2d_fixed_padding(h, W['c3'], 1))
  if fault == 'bn3_dx_twice':
    h = _GradTimes.apply(h, 2.0)
  main = B.batch_norm(h, *Bn['bn3'])
  if fault == 'shortcut_dropped':
    y = r(F.relu(main + 0.0 * shortcut))
  elif fault == 'shortcut_grad_unmasked':
    y = r(_AddReluUnmaskedShortcut.apply(main, shortcut))
  else:
    y = r(F.relu(main + shortcut))
  y.backward(B.nchw(dy, dtype))
  out = {'y': B.nhwc(y), 'dx': B.nhwc(x0.grad)}
  for k, t in W.items():
    out['dw_' + k] = B.hwio(t.grad)
  for k, (g, b) in Bn.items():
    out['dgamma_' + k], out['dbeta_' + k] = g.grad.detach(), b.grad.detach()
  return out


def _mutated_mobilenet_block(fault, x, dy, w_dw, w_pw, bn, stride=1, dtype=F64, rounding=True):
  r = B.rounder(rounding)
  Wd = B.leaf(w_dw.detach().to(dtype).permute(2, 3, 0, 1).contiguous())
  Wp = B.conv_weight(w_pw, dtype, rounding)
  Bn = {k: (B.leaf(g.to(dtype)), B.leaf(b.to(dtype))) for k, (g, b) in bn.items()}
  x0 = B.leaf(B.nchw(x, dtype))
  taps = Wd.transpose(2, 3) if fault == 'depthwise_taps_transposed' else Wd
  h = r(B.depthwise_conv2d_fixed_padding(r(x0), taps, stride))
  h = r(F.relu(B.batch_norm(h, *Bn['bn_a'])))
  h = r(B.conv2d_fixed_padding(h, Wp, 1))
  y = r(F.relu(B.batch_norm(h, *Bn['bn_b'])))
  y.backward(B.nchw(dy, dtype))
  out = {'y': B.nhwc(y), 'dx': B.nhwc(x0.grad), 'dw_pw': B.hwio(Wp.grad), 'dw_dw': Wd.grad.detach().permute(2, 3, 0, 1).contiguous()}
  for k, (g, b) in Bn.items():
    out['dgamma_' + k], out['dbeta_' + k] = g.grad.detach(), b.grad.detach()
  return out


def _mutated_head(fault, x, labels, w, bias, label_smoothing, dtype=F64, rounding=True):
  r = B.rounder(rounding)
  wl = B.leaf((w.to(torch.bfloat16) if rounding else w).to(dtype))
  b = B.leaf(bias.to(dtype))
  x0 = B.leaf(x.to(dtype))
  n, hh, ww, _ = x0.shape
  count = (hh + 1) * (ww + 1) if fault == 'avgpool_wrong_count' else hh * ww      # (the window a padded pooling would count)
  feat = r(r(x0).sum(dim=(1, 2)) / count)
  logits = r(r(feat @ wl) + r(b))
  loss = B.softmax_cross_entropy(logits, labels, label_smoothing)
  loss.backward()
  return {'y': loss.detach(), 'dx': x0.grad.detach(), 'dw_fc': wl.grad.detach(), 'dbias': b.grad.detach()}


def _figures(got, ref):
  return {k: B.rel_l2(got[k], ref[k]) for k in ref}


# (fault, projection, stride, cin, f, hw): the block kind each fault can occur in
_BOTTLENECK_MUTATION_CASES = [
    ('shortcut_dropped', False, 1, 64, 16, 12),
    ('shortcut_dropped', True, 2, 64, 32, 12),
    ('shortcut_after_conv1', True, 1, 16, 16, 12),
    ('shortcut_grad_unmasked', False, 1, 64, 16, 12),
    ('shortcut_grad_unmasked', True, 2, 64, 32, 12),
    ('proj_grad_odd_pixels', True, 2, 64, 32, 12),
    ('same_padding_on_strided_3x3', True, 2, 64, 32, 12),
    ('bn3_dx_twice', False, 1, 64, 16, 12),
    ('bn3_dx_twice', True, 2, 64, 32, 12),
]


def test_every_listed_fault_has_a_case():
  assert {c[0] for c in _BOTTLENECK_MUTATION_CASES} == set(BOTTLENECK_FAULTS)


@pytest.mark.parametrize('proj,stride', [(False, 1), (True, 1), (True, 2)])
def test_the_unmutated_copies_are_the_twins(proj, stride):
  """The copies the faults are seeded into compute what block_ref computes, bit for bit."""
  ops = _bottleneck_operands(7, 2, 12, 16 if stride == 1 and proj else 64, 16, stride, proj)
  a, b = B.bottleneck(*ops, stride=stride), _mutated_bottleneck(None, *ops, stride=stride)
  assert all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)
  ops = _mobilenet_operands(7, 2, 12, 16, 24, 2)
  a, b = B.mobilenet_block(*ops, stride=2), _mutated_mobilenet_block(None, *ops, stride=2)
  assert all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)
  ops = _head_operands(7, 5, 7, 24, 10)
  a, b = B.head(*ops, 0.1), _mutated_head(None, *ops, 0.1)
  assert all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)


@pytest.mark.parametrize('fault,proj,stride,cin,f,hw', _BOTTLENECK_MUTATION_CASES)
def test_bottleneck_fault_leaves_the_bound(fault, proj, stride, cin, f, hw):
  ops = _bottleneck_operands(11, 3, hw, cin, f, stride, proj)
  ref = B.bottleneck(*ops, stride=stride)
  floor = _figures(B.bottleneck(*ops, stride=stride, dtype=torch.float32), ref)
  assert max(floor.values()) <= B.BOUND / 8, floor            # the comparison itself is quiet on these operands
  fig = _figures(_mutated_bottleneck(fault, *ops, stride=stride), ref)
  print(fault, {k: '%.3g' % v for k, v in fig.items()})
  assert max(fig.values()) > B.BOUND, (fault, fig)


@pytest.mark.parametrize('stride,hw', [(1, 12), (2, 12), (2, 15)])
def test_transposed_depthwise_taps_leave_the_bound(stride, hw):
  ops = _mobilenet_operands(12, 3, hw, 16, 24, stride)
  ref = B.mobilenet_block(*ops, stride=stride)
  floor = _figures(B.mobilenet_block(*ops, stride=stride, dtype=torch.float32), ref)
  assert max(floor.values()) <= B.BOUND / 8, floor
  fig = _figures(_mutated_mobilenet_block('depthwise_taps_transposed', *ops, stride=stride), ref)
  assert max(fig.values()) > B.BOUND, fig


@pytest.mark.parametrize('eps', [0.0, 0.1])
def test_average_pool_wrong_count_leaves_the_bound(eps):
  ops = _head_operands(13, 8, 7, 64, 10)
  ref = B.head(*ops, eps)
  floor = _figures(B.head(*ops, eps, dtype=torch.float32), ref)
  assert max(floor.values()) <= B.BOUND / 8, floor
  fig = _figures(_mutated_head('avgpool_wrong_count', *ops, eps), ref)
  assert max(fig.values()) > B.BOUND, fig


def test_rel_l2_zero_reference_admits_only_zero():
  z = torch.zeros(4)
  assert B.rel_l2(z, z) == 0.0 and B.rel_l2(torch.tensor([0., 0., 1e-30, 0.]), z) == float('inf')
  assert abs(B.rel_l2(torch.tensor([3.0, 4.0]), torch.tensor([3.0, 0.0])) - 4.0 / 3.0) < 1e-15
