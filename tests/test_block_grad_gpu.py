"""Every residual and depthwise block, the stem and the head: the product's forward and backward against the float64
twin of the same block (tests/block_ref.py, checked on the CPU by tests/test_block_ref_cpu.py).

The kernels are pinned one by one elsewhere; what stands between them -- workloads/resnet50.py::_Bottleneck,
workloads/mobilenet_v1.py's block, and the autograd bridge (fork, conv_pair, _BnAddBnFn, MaskedAddendHolder,
BnApplyHolder, _BnReluMaxPoolFn) -- was only ever compared with itself under two knob settings, which a fault shared
by both settings passes: a shortcut taken from the wrong tensor, a projection gradient scattered to the wrong pixels,
a ReLU mask missing from the shortcut gradient, the wrong padding on the stride-2 3x3.  Here each block is built from
the product's own classes on a fresh graph, runs ONE forward and ONE backward, and every output -- the block output,
dX, the dense dW of every conv, dgamma / dbeta of every batch norm -- is compared with the twin on the same operands.

Why a tight bound holds here and not in tests/test_network_grad_gpu.py: the upstream gradient is i.i.d. N(0, 1) with a
per-channel mean of about zero, so batch norm's backward has no common mode to amplify, and one block has few stored
tensors.  Bound (block_ref.bound_note): relative L2 <= 2^-6 per tensor against the rounding-point twin; a tensor whose
reference is zero must be exactly zero.  2^-6 is far inside the chain bound of test_network_grad_gpu.py (relative L2
<= 0.15, ||dW|| within 5 %), the outer cap.  The floor -- the twin in fp32 arithmetic against the twin in float64,
reference code only -- and the figure against the plain (unrounded) float64 function are measured on the same operands
and attached with record_property; profiles/blockgrad/README.md holds the measured figures.

Cases: the smallest batch at which the route in question is still taken (256 CUs: bwdslice.hpp bs_plan wants four
32-row tiles per row group, bwd1x1.hpp 8 192 rows under "bwd1x1" = 2, rowstream.hpp 4 096 rows).  Every case ASSERTS its
route: the library is asked (ops.conv_bwd_takes_masked_addend / conv_bwd_takes_bn_apply), the armed hand-overs are
counted, and the backward entry points that ran are counted -- a case cannot quietly run the plain path.
"""
import collections

import pytest

torch = pytest.importorskip('torch')

from tests import block_ref as B  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SPARSITY = 0.8


# ---------------------------------------------------------------------------------------------------------------------
# operands and bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
  return torch.Generator(device=DEV).manual_seed(seed)


def _randn_bf16(gen, shape, relu=False):
  t = torch.randn(shape, generator=gen, device=DEV)
  return (t.relu() if relu else t).to(torch.bfloat16)


def _sparsify(layers, gen):
  """A random 80 %-sparse mask on every masked layer."""
  for lv in layers:
    lv.mask.assign((torch.rand(lv.mask.shape, generator=gen, device=DEV) >= SPARSITY).float())


def _set_bn(bns, gen):
  """gamma ~ U(0.5, 1.5), beta ~ 0.3 N(0, 1): bn3's zero-initialised gamma would switch the main branch off."""
  for bn in bns:
    bn.gamma.data.copy_(torch.rand(bn.channels, generator=gen, device=DEV) + 0.5)
    bn.beta.data.copy_(torch.randn(bn.channels, generator=gen, device=DEV) * 0.3)


def _masked_weights(layer):
  """mask * W, fp32, in the layer's own layout: the operand the twin rounds to the shadow the kernels read."""
  w = layer.weights.data.detach().clone()
  return w * layer.mask.data.reshape(w.shape) if layer.mask is not None else w


def _bn_pair(bn):
  return bn.gamma.data.detach().clone(), bn.beta.data.detach().clone()


class _Routes:
  """Counts the hand-overs made during a forward + backward and the backward entry points that ran."""

  def __init__(self):
    self.holders, self.calls = [], collections.Counter()

  def __enter__(self):
    from rigl_amd import ops, pruning_layers as PL
    self._ops, self._PL = ops, PL
    self._init0 = PL._HandOver.__init__
    self._saved = {k: getattr(ops, k) for k in ('conv_bwd', 'conv_bwd_grid', 'conv_bwd_bnapply', 'bn_add_bn_bwd',
                                                 'bn_relu_maxpool_bwd')}
    routes, init0 = self, self._init0

    def collecting(holder):
      init0(holder)
      routes.holders.append(holder)
    PL._HandOver.__init__ = collecting

    def counted(name, fn):
      def call(*a, **k):
        routes.calls[name] += 1
        if name == 'conv_bwd':
          if k.get('addend_bits') is not None:
            routes.calls['conv_bwd:masked_addend'] += 1
          if k.get('addend_sub') is not None and tuple(k['addend_sub']) != (1, 1):
            routes.calls['conv_bwd:sub_addend'] += 1
        return fn(*a, **k)
      return call
    for k, fn in self._saved.items():
      setattr(ops, k, counted(k, fn))
    return self

  def __exit__(self, *exc):
    self._PL._HandOver.__init__ = self._init0
    for k, fn in self._saved.items():
      setattr(self._ops, k, fn)

  def armed(self, cls):
    return sum(1 for h in self.holders if isinstance(h, cls) and h.armed)


def _compare(case, got, operands_twin, record_property):
  """``operands_twin(dtype, rounding)`` -> the twin's outputs.  Asserts the bound per tensor; records floor / product / plain."""
  ref = operands_twin(torch.float64, True)
  f32 = operands_twin(torch.float32, True)
  plain = operands_twin(torch.float64, False)
  assert set(got) == set(ref), (sorted(got), sorted(ref))
  fig = {}
  for k in sorted(ref):
    fig[k] = (B.rel_l2(f32[k], ref[k]), B.rel_l2(got[k], ref[k]), B.rel_l2(got[k], plain[k]))
    record_property('%s floor' % k, fig[k][0])
    record_property('%s product' % k, fig[k][1])
    record_property('%s product_vs_plain_fp64' % k, fig[k][2])
    print('BLOCKGRAD %s %s floor=%.3g product=%.3g plain=%.3g' % (case, k, *fig[k]))
  worst_floor, worst = max(v[0] for v in fig.values()), max(v[1] for v in fig.values())
  record_property('worst floor', worst_floor)
  record_property('worst product', worst)
  print('BLOCKGRAD %s WORST floor=%.3g product=%.3g plain=%.3g' % (case, worst_floor, worst, max(v[2] for v in fig.values())))
  # (relative L2 <= 2^-6 also keeps ||got|| within 1.6 % of ||ref||: inside the outer cap of 0.15 / 5 % with room to spare)
  assert B.BOUND < B.OUTER_REL and B.BOUND < B.OUTER_NORM
  bad = {k: v for k, v in fig.items() if not v[1] <= B.BOUND}
  assert not bad, '%s: (floor, product, vs plain fp64) outside relative L2 2^-6: %s' % (case, bad)


# ---------------------------------------------------------------------------------------------------------------------
# bottlenecks
# ---------------------------------------------------------------------------------------------------------------------
# group / block: the specs of workloads.shapes.resnet50_blocks; n, hw: the input [n, hw, hw, cin]; knobs: ops.tune_set.
# addend / apply: is the masked-addend hand-over (fork -> relu(bn3 + shortcut)) / bn3's apply on conv3's dY load armed;
# pair: conv_pair runs as one node; c1_masked: what rigl_conv2d_bwd_takes_masked_addend says for conv1 (for a pair block:
# is conv1 on the channel-sliced backward, which then takes the sub-sampled addend -- else the igemm epilogue does).
BCase = collections.namedtuple('BCase', 'name group block n hw knobs addend apply pair c1_masked')
BOTTLENECKS = [
    BCase('g1_identity_n3_rs_masked_bn3_on_load', 1, 1, 3, 56, {'bwd1x1': 2, 'rs_masked_addend': 2}, True, True, False, True),
    BCase('g1_identity_n2_plain_handovers', 1, 1, 2, 56, {}, False, False, False, False),
    BCase('g1_block0_n3_stride1_projection', 1, 0, 3, 56, {}, False, False, False, False),
    BCase('g2_block0_n3_pair_igemm_sub', 2, 0, 3, 56, {}, False, False, True, False),
    BCase('g2_block0_n6_pair_bwdslice_sub', 2, 0, 6, 56, {}, False, False, True, True),
    BCase('g2_identity_n11_bwdslice128', 2, 1, 11, 28, {}, True, False, False, True),
    BCase('g3_block0_n11_pair_bwdslice256', 3, 0, 11, 28, {}, False, False, True, True),
    BCase('g3_identity_n21_bwdslice256', 3, 1, 21, 14, {}, True, False, False, True),
    BCase('g4_block0_n11_pair_bwdslice512', 4, 0, 11, 14, {}, False, False, True, True),
    BCase('g4_identity_n21_bwdslice64', 4, 1, 21, 7, {}, True, False, False, True),
    BCase('g1_identity_n2_14x14_generic_bodies', 1, 1, 2, 14, {}, False, False, False, False),
]


@pytest.mark.parametrize('case', BOTTLENECKS, ids=[c.name for c in BOTTLENECKS])
def test_bottleneck_against_the_fp64_twin(case, record_property):
  from rigl_amd import ops, pruning_layers as PL, variables as V
  from rigl_amd.workloads import resnet50 as R, shapes as WS
  PL.set_init_seed(0)
  g = V.Graph(DEV)
  convs = next(cs for grp, n, cs in WS.resnet50_blocks() if grp == case.group and n == case.block)
  blk = R._Bottleneck(g, convs, 'threshold', 1e-4, 'blk')
  g.finalize()
  gen = _gen(1000 * case.group + 10 * case.n + case.hw)
  _sparsify(g.masked_layers(), gen)
  has_proj = blk.proj is not None
  bns = {'bn1': blk.bn1, 'bn2': blk.bn2, 'bn3': blk.bn3}
  cvs = {'c1': blk.c1.conv, 'c2': blk.c2.conv, 'c3': blk.c3.conv}
  if has_proj:
    bns['bn_proj'], cvs['proj'] = blk.proj_bn, blk.proj.conv
  _set_bn(bns.values(), gen)
  stride = blk.c2.stride
  cin = blk.c1.conv.cin
  x = _randn_bf16(gen, (case.n, case.hw, case.hw, cin), relu=True).requires_grad_(True)     # the previous block's ReLU output
  try:
    for k, v in case.knobs.items():
      ops.tune_set(k, v)
    # what the library says about this case's layers, under the case's knobs
    d1 = blk.c1.conv.desc_for(case.n, case.hw, case.hw)
    ho = (case.hw - 1) // stride + 1
    d3 = blk.c3.conv.desc_for(case.n, ho, ho)
    assert ops.conv_bwd_takes_masked_addend(d1) == case.c1_masked, 'conv1: the library plans another backward body at this batch'
    assert ops.conv_bwd_takes_bn_apply(d3) == case.apply, 'conv3: bn3\'s apply on the dY load is planned otherwise at this batch'
    if has_proj and not case.pair:
      assert not ops.conv_bwd_takes_masked_addend(blk.proj.conv.desc_for(case.n, case.hw, case.hw))
    with _Routes() as routes:
      y = blk(x, True)
      dy = _randn_bf16(gen, y.shape)
      y.backward(dy)
      torch.cuda.synchronize()
  finally:
    for k in case.knobs:
      ops.tune_unset(k)
  # the route this case claims
  assert all(h.grad is None and h.payload is None for h in routes.holders), 'a hand-over was filled and never taken'
  assert routes.armed(PL.MaskedAddendHolder) == int(case.addend) == routes.calls['conv_bwd:masked_addend']
  assert routes.armed(PL.BnApplyHolder) == int(case.apply) == routes.calls['conv_bwd_bnapply']
  assert routes.calls['conv_bwd_grid'] == int(case.pair) == routes.calls['conv_bwd:sub_addend']
  assert routes.calls['bn_add_bn_bwd'] == int(has_proj)
  assert routes.calls['conv_bwd'] + routes.calls['conv_bwd_grid'] + routes.calls['conv_bwd_bnapply'] == len(cvs)
  got = {'y': y.detach(), 'dx': x.grad}
  for k, c in cvs.items():
    got['dw_' + k] = c.weights.grad.detach().clone()
  for k, bn in bns.items():
    got['dgamma_' + k], got['dbeta_' + k] = bn.gamma.grad.detach().clone(), bn.beta.grad.detach().clone()
  w = {k: _masked_weights(c) for k, c in cvs.items()}
  bnp = {k: _bn_pair(bn) for k, bn in bns.items()}
  _compare(case.name, got, lambda dt, rnd: B.bottleneck(x.detach(), dy, w, bnp, stride=stride, dtype=dt, rounding=rnd), record_property)


# ---------------------------------------------------------------------------------------------------------------------
# MobileNet-v1 block
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,hw,c,f,stride', [(4, 28, 256, 256, 1), (4, 28, 256, 512, 2), (3, 15, 64, 128, 2)])
def test_mobilenet_block_against_the_fp64_twin(n, hw, c, f, stride, record_property):
  """(dw, bn_a, pw, bn_b) as MobileNetV1.__init__ makes them, wired as MobileNetV1.__call__ wires a block.  28 is even: fixed
  padding (one pixel in front) differs from tf 'SAME' (none in front) at stride 2; 15 is odd, where the last window ends on
  the padding; both convs leave the statistics partials of the batch norm behind them."""
  from rigl_amd import pruning_layers as PL, variables as V
  from rigl_amd.workloads import nn as gnn
  PL.set_init_seed(0)
  g = V.Graph(DEV)
  dw = gnn.DepthwiseConv2d(g, 'blk/depthwise_nxn', c, 3, stride)
  bn_a = gnn.BatchNorm(g, 'blk/depthwise_bn', c)
  pw = PL.MaskedConv2d(g, 'blk/contraction_1x1', c, f, (1, 1), (1, 1), 'SAME', 'threshold', 4e-5, PL.variance_scaling_initializer())
  g.modules['blk/contraction_1x1'] = pw
  bn_b = gnn.BatchNorm(g, 'blk/contraction_bn', f)
  g.finalize()
  gen = _gen(n * 100 + hw + c)
  _sparsify(g.masked_layers(), gen)
  _set_bn((bn_a, bn_b), gen)
  x = _randn_bf16(gen, (n, hw, hw, c), relu=True).requires_grad_(True)
  h_dw = dw(x, bn_stats=True)
  h_pw = pw(bn_a(h_dw, True, relu=True), bn_stats=True)
  y = bn_b(h_pw, True, relu=True)
  assert getattr(h_dw, 'bn_partials', None) is not None, 'the depthwise epilogue left no statistics partials'
  assert getattr(h_pw, 'bn_partials', None) is not None, 'the pointwise epilogue left no statistics partials'
  dy = _randn_bf16(gen, y.shape)
  y.backward(dy)
  torch.cuda.synchronize()
  got = {'y': y.detach(), 'dx': x.grad, 'dw_dw': dw.weights.grad.detach().clone(), 'dw_pw': pw.weights.grad.detach().clone()}
  for k, bn in (('bn_a', bn_a), ('bn_b', bn_b)):
    got['dgamma_' + k], got['dbeta_' + k] = bn.gamma.grad.detach().clone(), bn.beta.grad.detach().clone()
  w_dw, w_pw = dw.weights.data.detach().clone(), _masked_weights(pw)
  bnp = {'bn_a': _bn_pair(bn_a), 'bn_b': _bn_pair(bn_b)}
  _compare('mobilenet_n%d_%dx%d_%d_%d_s%d' % (n, hw, hw, c, f, stride), got,
           lambda dt, rnd: B.mobilenet_block(x.detach(), dy, w_dw, w_pw, bnp, stride=stride, dtype=dt, rounding=rnd), record_property)


# ---------------------------------------------------------------------------------------------------------------------
# ResNet-50 stem and head
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def resnet50_model():
  from rigl_amd import variables as V
  from rigl_amd.workloads import resnet50
  model = resnet50.ResNet50(V.Graph(DEV), seed=0)
  gen = _gen(50)
  _sparsify([model.stem.conv.vars, model.fc.vars], gen)
  _set_bn([model.stem_bn], gen)
  model.fc.bias.data.copy_(torch.randn(model.fc.units, generator=gen, device=DEV) * 0.1)
  return model


def test_resnet50_stem_against_the_fp64_twin(resnet50_model, record_property):
  """The model's own stem conv and batch norm through bn_relu_max_pool_3x3_s2_same, as ResNet50.__call__ runs them: 64 x 64
  images give a 32 x 32 conv output (a multiple of the direct stem kernel's 16 x 16 tiles) and the fused BN-ReLU-pool node."""
  from rigl_amd.workloads import nn as gnn
  model = resnet50_model
  gen = _gen(51)
  x = _randn_bf16(gen, (2, 64, 64, 3))
  with _Routes() as routes:
    y = gnn.bn_relu_max_pool_3x3_s2_same(model.stem_bn, model.stem(x), True)
    assert tuple(y.shape) == (2, 16, 16, 64)
    dy = _randn_bf16(gen, y.shape)
    y.backward(dy)
    torch.cuda.synchronize()
  assert routes.calls['bn_relu_maxpool_bwd'] == 1, 'the stem tail did not run as the fused node'
  assert routes.calls['conv_bwd'] == 1
  bn = model.stem_bn
  got = {'y': y.detach(), 'dw_stem': model.stem.conv.weights.grad.detach().clone(),
         'dgamma_bn': bn.gamma.grad.detach().clone(), 'dbeta_bn': bn.beta.grad.detach().clone()}
  w, bnp = _masked_weights(model.stem.conv), {'bn': _bn_pair(bn)}
  _compare('resnet50_stem_n2_64x64', got, lambda dt, rnd: B.resnet_stem(x, dy, w, bnp, dtype=dt, rounding=rnd), record_property)


def _head_case(name, fc, x, labels, eps, record_property):
  from rigl_amd.workloads import nn as gnn
  fc.bias.grad.zero_()                                       # (autograd accumulates into the bias' slice of the arena)
  loss = gnn.softmax_cross_entropy(fc(gnn.global_avg_pool(x)), labels, eps)
  loss.backward()
  torch.cuda.synchronize()
  got = {'y': loss.detach(), 'dx': x.grad, 'dw_fc': fc.weights.grad.detach().clone(), 'dbias': fc.bias.grad.detach().clone()}
  w, bias = _masked_weights(fc), fc.bias.data.detach().clone()
  _compare(name, got, lambda dt, rnd: B.head(x.detach(), labels, w, bias, eps, dtype=dt, rounding=rnd), record_property)


@pytest.mark.parametrize('eps', [0.1, 0.0])
def test_resnet50_head_against_the_fp64_twin(resnet50_model, eps, record_property):
  """The model's own final_dense behind global_avg_pool, under softmax_cross_entropy, as ResNet50.loss runs them."""
  gen = _gen(52)
  x = _randn_bf16(gen, (8, 7, 7, 2048), relu=True).requires_grad_(True)
  labels = torch.randint(0, 1000, (8,), generator=gen, device=DEV)
  _head_case('resnet50_head_n8_7x7_2048_1000_eps%g' % eps, resnet50_model.fc, x, labels, eps, record_property)


@pytest.mark.parametrize('eps', [0.1, 0.0])
def test_small_head_against_the_fp64_twin(eps, record_property):
  """37 rows of 10 classes: an odd batch and a class count the MFMA kernels do not take (the direct kernels run)."""
  from rigl_amd import pruning_layers as PL, variables as V
  PL.set_init_seed(0)
  g = V.Graph(DEV)
  fc = PL.MaskedDense(g, 'head/final_dense', 64, 10, True, 'threshold', 1e-4, PL.random_normal_initializer(0.1))
  g.modules['head/final_dense'] = fc
  g.finalize()
  gen = _gen(53)
  _sparsify([fc.vars], gen)
  fc.bias.data.copy_(torch.randn(10, generator=gen, device=DEV) * 0.1)
  x = _randn_bf16(gen, (37, 8, 8, 64), relu=True).requires_grad_(True)
  labels = torch.randint(0, 10, (37,), generator=gen, device=DEV)
  _head_case('small_head_n37_8x8_64_10_eps%g' % eps, fc, x, labels, eps, record_property)
