"""Chained in-situ parity along whole networks.

tests/test_network_grad_gpu.py compares the END of a 22-layer backward pass with stock ops and has to allow 15 %: two
correct bf16 implementations differ by half-ulps in every activation gradient and batch norm amplifies those.  Here the
errors cannot compound: a stock-op reference of the network (fp64 arithmetic, a bf16 rounding wherever the HIP path stores
a bf16 tensor) runs ONCE and records, for every conv and every batch-norm node, the tensors that node consumed and the
gradient that arrived at its output; then each HIP kernel is fed THE REFERENCE'S tensors and held to the per-kernel bound

  conv fwd / dgrad   |got - ref| <= 2^-8 |ref| + 1e-5 sum|a||b|     (bf16 output rounding + fp32 accumulation)
  conv wgrad         |got - ref| <= 1e-5 sum|a||b|
  batch norm y, dx   |got - ref| <= 2^-8 |ref| + 1e-5 (sum of the magnitudes of the terms of the element's formula)
  batch norm dgamma  |got - ref| <= 1e-5 sum |dz xhat|,   dbeta: 1e-5 sum |dz|      (fp32-accumulation bounds)

so a wrong scale confined to a few low-energy channels of one layer -- invisible in a 15 % band -- fails its own node.
Networks: the 22-layer WideResNet of BASELINE config 2 (16 / 32 / 64 channels: the igemm bodies) and a stack of two
ResNet-50 group-3 bottleneck blocks at 14x14 (256 / 1024 channels: the ping-pong forward, the shared ping-pong backward
launch and its 256x256 weight-gradient tiles), and two group-1 bottleneck blocks at 56x56 (64 / 256 channels: the
slab-resident 3x3 kernels of c3x3.hpp, the single-pass 1x1 backward of bwd1x1.hpp, the projection shortcut) whose conv
epilogues' statistics partials are ALSO fed to the batch norm that follows (VERDICT r3, weak #1a).  The checker (stock
ops in fp64, tests/convref.py) is test infrastructure.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
import torch.nn.functional as F  # noqa: E402

from tests import convref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS = 1e-5


class _RoundBF16(torch.autograd.Function):
  """bf16 rounding of a tensor in the forward AND of its gradient in the backward pass (values stay fp64)."""

  @staticmethod
  def forward(ctx, x):
    return x.to(torch.bfloat16).to(x.dtype)

  @staticmethod
  def backward(ctx, g):
    return g.to(torch.bfloat16).to(g.dtype)


rnd = _RoundBF16.apply


class Recorder:
  """Stock-op network pieces in fp64 (NCHW) that remember what each node saw."""

  def __init__(self):
    self.convs, self.bns, self.dws = [], [], []

  def conv(self, name, x, w_hwio_f32, k, stride, pads):
    """pads = (top, left, bottom, right).  Returns the bf16-rounded output."""
    xi = (x * 1.0)                                   # this consumer's own copy: its .grad is THIS conv's dX alone
    if xi.requires_grad:                             # (the network input has no gradient)
      xi.retain_grad()
    w = w_hwio_f32.to(torch.bfloat16).double().clone().requires_grad_(True)     # the shadow the kernels read
    pt, pl, pb, pr = pads
    y_raw = F.conv2d(F.pad(xi, (pl, pr, pt, pb)), w.permute(3, 2, 0, 1), stride=stride)
    y_raw.retain_grad()                              # its .grad is the bf16-rounded gradient the conv's backward consumes
    self.convs.append(dict(name=name, x=xi, w=w, w32=w_hwio_f32, y=y_raw, k=k, stride=stride, pads=pads))
    return rnd(y_raw)

  def depthwise(self, name, x, w_hwc_f32, stride, pads):
    """A grouped (channel multiplier 1) conv; the kernels read the fp32 weights [kh,kw,C] as they are.  pads = (top, left,
    bottom, right).  Returns the bf16-rounded output."""
    xi = (x * 1.0)
    if xi.requires_grad:
      xi.retain_grad()
    w = w_hwc_f32.double().clone().requires_grad_(True)
    pt, pl, pb, pr = pads
    y_raw = F.conv2d(F.pad(xi, (pl, pr, pt, pb)), w.permute(2, 0, 1).unsqueeze(1), stride=stride, groups=w.shape[-1])
    y_raw.retain_grad()
    self.dws.append(dict(name=name, x=xi, w=w, w32=w_hwc_f32, y=y_raw, stride=stride, pads=pads))
    return rnd(y_raw)

  def bn(self, name, x, gamma, beta, relu, residual=None):
    xi = (x * 1.0)
    xi.retain_grad()
    ri = None
    if residual is not None:
      ri = residual * 1.0
      ri.retain_grad()
    g64 = gamma.double().clone().requires_grad_(True)
    b64 = beta.double().clone().requires_grad_(True)
    y = F.batch_norm(xi, None, None, g64, b64, True, 0.1, EPS)
    if ri is not None:
      y = y + ri
    if relu:
      y = F.relu(y)
    y.retain_grad()
    self.bns.append(dict(name=name, x=xi, res=ri, gamma=gamma, beta=beta, g64=g64, b64=b64, y=y, relu=relu))
    return rnd(y)


def _nhwc_bf16(t):
  return t.detach().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)


def check_conv_node(nd):
  """The HIP forward / dgrad / wgrad of one conv on the reference's tensors against tests/convref.py."""
  from rigl_amd import ops
  x = _nhwc_bf16(nd['x'])
  dy = _nhwc_bf16(nd['y'].grad)
  assert torch.equal(dy.double(), nd['y'].grad.detach().permute(0, 2, 3, 1)), 'the recorded gradient is not bf16-valued'
  N, H, W, Cin = x.shape
  _, Ho, Wo, Cout = dy.shape
  k, s = nd['k'], nd['stride']
  pt, pl = nd['pads'][0], nd['pads'][1]
  n = k * k * Cin * Cout
  hwio = torch.empty(n, dtype=torch.bfloat16, device=DEV)
  ohwi = torch.empty(n, dtype=torch.bfloat16, device=DEV)
  ops.pack_weights(nd['w32'].reshape(-1).contiguous(), None, k * k * Cin, Cout, hwio, ohwi)
  wm = hwio.float().reshape(k, k, Cin, Cout)
  assert torch.equal(wm.double(), nd['w'].detach()), 'packed shadow != the reference weights'
  d = ops.conv_desc(N, H, W, Cin, Cout, k, k, s, pt, pl, Ho, Wo)
  has_dx = Cin % 8 == 0
  want = ('y', 'dx', 'dw') if has_dx else ('y', 'dw')
  ref = convref.conv_fp64(x, wm, dy, s, pt, pl, Ho, Wo, want)
  ab = convref.conv_fp64(x.abs(), wm.abs(), dy.abs(), s, pt, pl, Ho, Wo, want)
  # (the matrix-product reference must agree with the stock-op graph it is standing in for)
  assert float((ref['y'] - nd['y'].detach().permute(0, 2, 3, 1)).abs().max()) <= 1e-9 * float(ab['y'].max() + 1e-30)
  worst = 0.0
  if Cout % 8 == 0:
    y = ops.conv_fwd(d, x, ohwi)
    worst = max(worst, convref.check_close(nd['name'] + ' fwd', y, ref['y'], ab['y'], 1e-5, 2.0 ** -8))
    dw = torch.empty(n, dtype=torch.float32, device=DEV)
    dx = ops.conv_bwd(d, x, dy, hwio, dw, need_dx=has_dx)
    worst = max(worst, convref.check_close(nd['name'] + ' wgrad', dw.reshape(k, k, Cin, Cout), ref['dw'], ab['dw'], 1e-5))
    if has_dx:
      worst = max(worst, convref.check_close(nd['name'] + ' dgrad', dx, ref['dx'], ab['dx'], 1e-5, 2.0 ** -8))
      gx = nd['x'].grad.detach().permute(0, 2, 3, 1)
      assert float((ref['dx'] - gx).abs().max()) <= 1e-9 * float(ab['dx'].max() + 1e-30)
  return worst


def check_bn_node(nd, sum_terms=False):
  """The HIP batch norm (+ residual)(+ ReLU) forward and backward on the reference's tensors.

  ``sum_terms``: dX = a (dz - dbeta / M - xhat dgamma / M) is held to its bound twice instead of once -- against the same
  formula evaluated with the kernel's own dbeta / dgamma (each held to its fp32 bound just before), with the bound below
  (the apply pass alone), and against the fp64 reference with the magnitudes of the SUMMED terms, sum|dz| / M and
  |xhat| sum|dz xhat| / M, in place of |dbeta| / M and |xhat dgamma| / M (fp32 sums to 1e-5 of sum|terms|, as above).
  For long channels whose sums cancel (MobileNet-v1, 1.6 M rows: |dbeta| ~ 1e-5 sum|dz|) no fp32 reduction of dbeta
  is within 1e-5 |dbeta|, so the single bound on the reference's own sums would hold the kernel to more than fp32."""
  from rigl_amd import ops
  x = _nhwc_bf16(nd['x'])
  res = _nhwc_bf16(nd['res']) if nd['res'] is not None else None
  C = x.shape[-1]
  M = x.numel() // C
  gamma, beta = nd['gamma'].float().contiguous(), nd['beta'].float().contiguous()
  rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
  relu = nd['relu']
  out = ops.bn_fwd(x, gamma, beta, rm, rv, 0.1, EPS, relu, residual=res, want_relu_bits=relu and res is not None)
  y_hip, saved = out[0], out[1]
  bits = out[2] if len(out) > 2 else None
  # fp64 reference of the same formulas on the same bf16 inputs
  xd = x.double().reshape(M, C)
  mean = xd.mean(0)
  var = (xd * xd).mean(0) - mean * mean
  invstd = 1.0 / torch.sqrt(var.clamp_min(0) + EPS)
  xhat = (xd - mean) * invstd
  g64, b64 = gamma.double(), beta.double()
  pre = xhat * g64 + b64
  mag = xhat.abs() * g64.abs() + b64.abs()
  if res is not None:
    rd = res.double().reshape(M, C)
    pre = pre + rd
    mag = mag + rd.abs()
  y_ref = pre.clamp_min(0) if relu else pre
  assert float((y_ref.reshape(x.shape) - nd['y'].detach().permute(0, 2, 3, 1)).abs().max()) <= 1e-9 * float(mag.max())
  worst = convref.check_close(nd['name'] + ' y', y_hip.reshape(M, C), y_ref, mag, 1e-5, 2.0 ** -8)
  # saved statistics: mean within 1e-6 of the data scale, invstd relatively
  sm, si = saved[0].double(), saved[1].double()
  assert float(((sm - mean).abs() / (xd.abs().mean(0) + 1e-12)).max()) <= 1e-5, nd['name'] + ' saved mean'
  assert float(((si - invstd).abs() / invstd).max()) <= 1e-5, nd['name'] + ' saved invstd'
  # backward: the gradient that arrived at the node's output in the reference; the ReLU mask is the REFERENCE's
  dy = _nhwc_bf16(nd['y'].grad)
  dyd = dy.double().reshape(M, C)
  on = (y_ref > 0) if relu else torch.ones_like(y_ref, dtype=torch.bool)
  dz = torch.where(on, dyd, torch.zeros_like(dyd))
  dbeta = dz.sum(0)
  dgamma = (dz * xhat).sum(0)
  a = g64 * invstd
  dx_ref = a * (dz - dbeta / M - xhat * dgamma / M)
  dx_mag = a.abs() * (dz.abs() + dbeta.abs() / M + xhat.abs() * dgamma.abs() / M)
  y_mask = y_ref.reshape(x.shape).to(torch.bfloat16) if relu else None          # bf16(y) > 0  <=>  y > 0 (no flush to zero)
  if relu:
    assert bool(((y_mask.double() > 0) == on.reshape(x.shape)).all())
  dg = torch.empty(C, dtype=torch.float32, device=DEV)
  db = torch.empty(C, dtype=torch.float32, device=DEV)
  dx_hip, dres = ops.bn_bwd(x, y_mask, dy, gamma, saved, relu, dg, db, want_dres=res is not None)
  del bits
  worst = max(worst, convref.check_close(nd['name'] + ' dbeta', db, dbeta, dz.abs().sum(0), 1e-5))
  worst = max(worst, convref.check_close(nd['name'] + ' dgamma', dg, dgamma, (dz * xhat).abs().sum(0), 1e-5))
  if sum_terms:
    dbk, dgk = db.double(), dg.double()
    dx_k = a * (dz - dbk / M - xhat * dgk / M)
    mag_k = a.abs() * (dz.abs() + dbk.abs() / M + xhat.abs() * dgk.abs() / M)
    worst = max(worst, convref.check_close(nd['name'] + ' dx (kernel sums)', dx_hip.reshape(M, C), dx_k, mag_k, 1e-5, 2.0 ** -8))
    del dx_k, mag_k
    dx_mag = a.abs() * (dz.abs() + dz.abs().sum(0) / M + xhat.abs() * (dz * xhat).abs().sum(0) / M)
  worst = max(worst, convref.check_close(nd['name'] + ' dx', dx_hip.reshape(M, C), dx_ref, dx_mag, 1e-5, 2.0 ** -8))
  if res is not None:
    assert torch.equal(dres.reshape(M, C).double(), dz), nd['name'] + ': the residual gradient is the masked gradient, exactly'
  # ... and the recorded graph agrees with these formulas (the reference's own backward)
  assert float((nd['g64'].grad - dgamma).abs().max()) <= 1e-9 * float((dz * xhat).abs().sum(0).max() + 1e-30)
  gx = nd['x'].grad.detach().permute(0, 2, 3, 1).reshape(M, C)
  assert float((gx - dx_ref).abs().max()) <= 1e-9 * float(dx_mag.max() + 1e-30)
  return worst


def _same_pads(h, w, k, stride):
  """TF 'SAME': the extra pixel goes to the bottom / right."""
  if k == 1:
    return (0, 0, 0, 0)
  th = max((-(-h // stride) - 1) * stride + k - h, 0)
  tw = max((-(-w // stride) - 1) * stride + k - w, 0)
  return (th // 2, tw // 2, th - th // 2, tw - tw // 2)


def test_wrn22_every_conv_and_batch_norm_node_on_the_reference_tensors():
  from rigl_amd import sparse_utils, variables as V
  from rigl_amd.workloads import wide_resnet
  g = V.reset_default_graph(DEV)
  model = wide_resnet.WideResNet(g, depth=22, width=1)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
  gen = torch.Generator(device=DEV).manual_seed(3)
  for mod in g.modules.values():
    if hasattr(mod, 'gamma'):
      mod.gamma.data.copy_(1.0 + 0.2 * torch.randn(mod.channels, generator=gen, device=DEV))
      mod.beta.data.copy_(0.1 * torch.randn(mod.channels, generator=gen, device=DEV))
  x_nhwc, labels = wide_resnet.synthetic_batch(128, DEV)
  rec = Recorder()

  def w_of(layer):
    w = layer.weights.data.float()
    if layer.mask is not None:
      w = w * layer.mask.data.float().reshape(w.shape)
    return w.contiguous()

  def conv(layer, x, k):
    s = layer.strides[0]
    pads = _same_pads(x.shape[2], x.shape[3], k, s) if k == 3 else (0, 0, 0, 0)
    return rec.conv(layer.scope, x, w_of(layer), k, s, pads)

  def bn_relu(bn, name, x):
    return rec.bn(name, x, bn.gamma.data, bn.beta.data, True)

  net = conv(model.stem, x_nhwc.double().permute(0, 3, 1, 2), 3)
  for i, b in enumerate(model.blocks):
    skip = net
    net = bn_relu(b['bn_a'], 'block%d/bn_a' % i, net)
    if 'skip' in b:
      skip = conv(b['skip'], net, 1)
    net = conv(b['conv1'], net, 3)
    net = bn_relu(b['bn_b'], 'block%d/bn_b' % i, net)
    net = conv(b['conv2'], net, 3)
    net = rnd(net + skip)
  net = bn_relu(model.final_bn, 'final_bn', net)
  feat = rnd(net.mean(dim=(2, 3)))
  wl = w_of(model.logits).to(torch.bfloat16).double()
  logits = rnd(feat @ wl + model.logits.bias.data.double())
  F.cross_entropy(logits, labels).backward()
  assert len(rec.convs) == 21 and len(rec.bns) == 19
  worst = 0.0
  for nd in rec.convs:
    worst = max(worst, check_conv_node(nd))
  for nd in rec.bns:
    worst = max(worst, check_bn_node(nd))
  print('wrn22 chained: %d conv + %d batch-norm nodes, worst error / bound %.3f' % (len(rec.convs), len(rec.bns), worst))
  assert worst <= 1.0


def test_resnet50_group3_bottlenecks_every_node_on_the_reference_tensors():
  """Two group-3 bottleneck blocks (1x1 1024->256, 3x3 256->256, 1x1 256->1024, identity shortcut; resnet_model.py:456-501)
  at 14x14, batch 64: the shapes whose forward runs on the 128x256 ping-pong tile and whose backward runs the shared
  ping-pong launch (256x256 dgrad tiles next to the 256x256 weight-gradient tiles, split-K slabs + reduce)."""
  gen = torch.Generator(device=DEV).manual_seed(11)
  B, HW = 64, 14
  rec = Recorder()

  def rand_w(k, cin, cout):
    w = torch.randn(k, k, cin, cout, generator=gen, device=DEV) * (2.0 / (k * k * cin)) ** 0.5
    m = (torch.rand(k, k, cin, cout, generator=gen, device=DEV) < 0.2).float()       # 80 % sparse, like the ERK layers
    return (w * m).contiguous()

  def bn_params(c):
    return (1.0 + 0.2 * torch.randn(c, generator=gen, device=DEV)), 0.1 * torch.randn(c, generator=gen, device=DEV)

  x0 = torch.randn(B, 1024, HW, HW, generator=gen, device=DEV).to(torch.bfloat16).double()
  net = F.relu(x0).requires_grad_(True)
  for blk in range(2):
    shortcut = net
    t = rec.conv('b%d/c1' % blk, net, rand_w(1, 1024, 256), 1, 1, (0, 0, 0, 0))
    t = rec.bn('b%d/bn1' % blk, t, *bn_params(256), True)
    t = rec.conv('b%d/c2' % blk, t, rand_w(3, 256, 256), 3, 1, (1, 1, 1, 1))
    t = rec.bn('b%d/bn2' % blk, t, *bn_params(256), True)
    t = rec.conv('b%d/c3' % blk, t, rand_w(1, 256, 1024), 1, 1, (0, 0, 0, 0))
    net = rec.bn('b%d/bn3' % blk, t, *bn_params(1024), True, residual=shortcut)
  r = torch.randn(net.shape, generator=gen, device=DEV).double()
  (net * r).sum().backward()
  worst = 0.0
  for nd in rec.convs:
    worst = max(worst, check_conv_node(nd))
  for nd in rec.bns:
    worst = max(worst, check_bn_node(nd))
  print('resnet50 group-3 chained: %d conv + %d batch-norm nodes, worst error / bound %.3f' % (len(rec.convs), len(rec.bns), worst))
  assert worst <= 1.0


def check_stats_feed(cv, bn):
  """The conv epilogue's batch-norm partials (rigl_masked_conv2d_fwd_stats) feeding the REAL batch norm that follows it:
  the conv runs on the reference's input, its own bf16 output and partials go into rigl_bn_fwd_stats, and the result must
  be what the batch norm computes from that output by its own statistics pass -- scale / shift to 1e-5 of their
  magnitude (fp32 partial sums in another order), y within one bf16 ulp."""
  from rigl_amd import ops
  x = _nhwc_bf16(cv['x'])
  N, H, W, Cin = x.shape
  k, s = cv['k'], cv['stride']
  pt, pl = cv['pads'][0], cv['pads'][1]
  Cout = cv['w32'].shape[-1]
  Ho, Wo = cv['y'].shape[2], cv['y'].shape[3]
  n = k * k * Cin * Cout
  hwio = torch.empty(n, dtype=torch.bfloat16, device=DEV)
  ohwi = torch.empty(n, dtype=torch.bfloat16, device=DEV)
  ops.pack_weights(cv['w32'].reshape(-1).contiguous(), None, k * k * Cin, Cout, hwio, ohwi)
  d = ops.conv_desc(N, H, W, Cin, Cout, k, k, s, pt, pl, Ho, Wo)
  y, part = ops.conv_fwd(d, x, ohwi, stats=True)
  assert part is not None and part.shape[0] == d._stats_parts
  _check_bn_on_partials(cv['name'], bn, y, part)


def _check_bn_on_partials(src, bn, y, part):
  """rigl_bn_fwd_stats on a producer's bf16 output ``y`` with that producer's partials against the same batch norm with its
  own statistics pass over ``y``."""
  from rigl_amd import ops
  Cout = y.shape[-1]
  gamma, beta = bn['gamma'].float().contiguous(), bn['beta'].float().contiguous()
  relu = bn['relu'] and bn['res'] is None
  outs = []
  for p in (None, part):
    rm, rv = torch.zeros(Cout, device=DEV), torch.ones(Cout, device=DEV)
    o = ops.bn_fwd(y, gamma, beta, rm, rv, 0.1, EPS, relu, partials=p)
    outs.append((o[0], o[1], rm, rv))
  (y0, s0, rm0, rv0), (y1, s1, rm1, rv1) = outs
  for a, b, what in ((s0[0], s1[0], 'mean'), (s0[1], s1[1], 'invstd'), (s0[2], s1[2], 'scale'), (s0[3], s1[3], 'shift'),
                     (rm0, rm1, 'moving mean'), (rv0, rv1, 'moving variance')):
    tol = 1e-5 * float(a.abs().max()) + 1e-7
    assert float((a - b).abs().max()) <= tol, '%s -> %s: %s from the epilogue partials' % (src, bn['name'], what)
  diff = (y0.float() - y1.float()).abs()
  assert float((diff / (y0.float().abs() * 2.0 ** -7 + 1e-6)).max()) <= 1.0, 'y differs by more than one bf16 ulp'
  assert float((diff > 0).float().mean()) <= 0.01


def test_resnet50_group1_bottlenecks_every_node_on_the_reference_tensors():
  """Two group-1 bottleneck blocks at 56x56, batch 24 (resnet_model.py:456-501): block 0 with the projection shortcut
  (1x1 64->256 + batch norm), block 1 with the identity shortcut.  Their kernels: 1x1 64->256 and 64->64 on the single-pass
  backward (bwd1x1.hpp), 3x3 64->64 on the slab-resident kernels (c3x3.hpp), 1x1 256->64 on the igemm bodies -- every
  conv and batch-norm node on the reference's tensors, and every conv's statistics partials fed to its batch norm."""
  gen = torch.Generator(device=DEV).manual_seed(13)
  B, HW = 24, 56
  rec = Recorder()

  def rand_w(k, cin, cout):
    w = torch.randn(k, k, cin, cout, generator=gen, device=DEV) * (2.0 / (k * k * cin)) ** 0.5
    m = (torch.rand(k, k, cin, cout, generator=gen, device=DEV) < 0.2).float()
    return (w * m).contiguous()

  def bn_params(c):
    return (1.0 + 0.2 * torch.randn(c, generator=gen, device=DEV)), 0.1 * torch.randn(c, generator=gen, device=DEV)

  x0 = torch.randn(B, 64, HW, HW, generator=gen, device=DEV).to(torch.bfloat16).double()
  net = F.relu(x0).requires_grad_(True)
  pairs = []

  def conv_bn(name, x, k, cin, cout, relu, residual=None):
    pad = (1, 1, 1, 1) if k == 3 else (0, 0, 0, 0)
    t = rec.conv(name, x, rand_w(k, cin, cout), k, 1, pad)
    t = rec.bn(name + '/bn', t, *bn_params(cout), relu, residual=residual)
    pairs.append((len(rec.convs) - 1, len(rec.bns) - 1))
    return t
  for blk, cin in enumerate((64, 256)):
    shortcut = conv_bn('b%d/proj' % blk, net, 1, cin, 256, False) if blk == 0 else net
    t = conv_bn('b%d/c1' % blk, net, 1, cin, 64, True)
    t = conv_bn('b%d/c2' % blk, t, 3, 64, 64, True)
    net = conv_bn('b%d/c3' % blk, t, 1, 64, 256, True, residual=shortcut)
  r = torch.randn(net.shape, generator=gen, device=DEV).double()
  (net * r).sum().backward()
  assert len(rec.convs) == 7 and len(rec.bns) == 7
  worst = 0.0
  for nd in rec.convs:
    worst = max(worst, check_conv_node(nd))
  for nd in rec.bns:
    worst = max(worst, check_bn_node(nd))
  for ci, bi in pairs:
    check_stats_feed(rec.convs[ci], rec.bns[bi])
  print('resnet50 group-1 chained: %d conv + %d batch-norm nodes, worst error / bound %.3f' % (len(rec.convs), len(rec.bns), worst))
  assert worst <= 1.0


def _dw_desc(nd):
  from rigl_amd import ops
  N, C, H, W = nd['x'].shape
  Ho, Wo = nd['y'].shape[2], nd['y'].shape[3]
  return ops.conv_desc(N, H, W, C, C, 3, 3, nd['stride'], nd['pads'][0], nd['pads'][1], Ho, Wo)


def check_dw_node(nd):
  """The HIP depthwise forward / dgrad / wgrad on the reference's tensors against tests/convref.py's depthwise_fp64, and that
  reference against the recorded graph (grouped F.conv2d and its autograd) to 1e-9."""
  from rigl_amd import ops
  x = _nhwc_bf16(nd['x'])
  dy = _nhwc_bf16(nd['y'].grad)
  assert torch.equal(dy.double(), nd['y'].grad.detach().permute(0, 2, 3, 1)), 'the recorded gradient is not bf16-valued'
  _, Ho, Wo, _ = dy.shape
  s, pt, pl = nd['stride'], nd['pads'][0], nd['pads'][1]
  w = nd['w32'].contiguous()
  wd = w.reshape(-1)
  d = _dw_desc(nd)
  ref = convref.depthwise_fp64(x, w, dy, s, pt, pl, Ho, Wo)
  ab = convref.depthwise_fp64(x.abs(), w.abs(), dy.abs(), s, pt, pl, Ho, Wo)
  assert float((ref['y'] - nd['y'].detach().permute(0, 2, 3, 1)).abs().max()) <= 1e-9 * float(ab['y'].max() + 1e-30)
  assert float((ref['dx'] - nd['x'].grad.detach().permute(0, 2, 3, 1)).abs().max()) <= 1e-9 * float(ab['dx'].max() + 1e-30)
  assert float((ref['dw'] - nd['w'].grad).abs().max()) <= 1e-9 * float(ab['dw'].max() + 1e-30)
  y = ops.depthwise_fwd(d, x, wd)
  worst = convref.check_close(nd['name'] + ' fwd', y, ref['y'], ab['y'], 1e-5, 2.0 ** -8)
  dx = ops.depthwise_dgrad(d, dy, wd)
  worst = max(worst, convref.check_close(nd['name'] + ' dgrad', dx, ref['dx'], ab['dx'], 1e-5, 2.0 ** -8))
  dw = torch.empty(wd.numel(), dtype=torch.float32, device=DEV)
  ops.depthwise_wgrad(d, x, dy, dw)
  worst = max(worst, convref.check_close(nd['name'] + ' wgrad', dw, ref['dw'].reshape(-1), ab['dw'].reshape(-1), 1e-5))
  return worst


def check_dw_stats_feed(dw, bn):
  """check_stats_feed for the depthwise forward: its statistics partials (rigl_depthwise_conv2d_fwd_stats) feeding bn_a."""
  from rigl_amd import ops
  x = _nhwc_bf16(dw['x'])
  y, part = ops.depthwise_fwd(_dw_desc(dw), x, dw['w32'].contiguous().reshape(-1), stats=True)
  assert part is not None, dw['name'] + ': no statistics epilogue'
  _check_bn_on_partials(dw['name'], bn, y, part)


def _record_mobilenet_v1(batch, dev):
  """MobileNet-v1 of BASELINE config 5 (bench.py's model, seed and uniform 90 % masks on the pointwise convs and
  final_dense; stem and depthwise convs dense) as a recorded fp64 stock-op graph at 224 x 224, with random batch-norm
  affine parameters, backpropagated from the cross-entropy of its logits.  Returns (recorder, statistics feeds)."""
  from rigl_amd import sparse_utils, variables as V
  from rigl_amd.workloads import mobilenet_v1
  g = V.reset_default_graph(dev)
  model = mobilenet_v1.MobileNetV1(g, seed=0)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'random', 0.9, {})()
  gen = torch.Generator(device=dev).manual_seed(5)
  bns = [model.stem_bn] + [b for blk in model.blocks for b in (blk[1], blk[3])]
  for bn in bns:
    c = bn.gamma.data.numel()
    bn.gamma.data.copy_(1.0 + 0.2 * torch.randn(c, generator=gen, device=dev))
    bn.beta.data.copy_(0.1 * torch.randn(c, generator=gen, device=dev))
  images, labels = mobilenet_v1.synthetic_batch(batch, dev)
  rec = Recorder()
  feeds = []

  def w_of(layer):
    w = layer.weights.data.float()
    if layer.mask is not None:
      w = w * layer.mask.data.float().reshape(w.shape)
    return w.contiguous()

  def bn_relu(bn, name, x):
    return rec.bn(name, x, bn.gamma.data, bn.beta.data, True)

  # fixed padding 1 / 1 + VALID for the 3x3 stem and the stride-2 depthwise convs, SAME (also 1 / 1) at stride 1
  net = rec.conv('initial_conv', images.double().permute(0, 3, 1, 2), w_of(model.stem), 3, 2, (1, 1, 1, 1))
  net = bn_relu(model.stem_bn, 'initial_bn', net)
  feeds.append(('conv', len(rec.convs) - 1, len(rec.bns) - 1))
  for i, (dw, bn_a, pw, bn_b) in enumerate(model.blocks):
    net = rec.depthwise('depthwise_nxn_%d' % i, net, dw.weights.data.float().reshape(3, 3, -1), dw.stride, (1, 1, 1, 1))
    net = bn_relu(bn_a, 'depthwise_bn_%d' % i, net)
    feeds.append(('dw', len(rec.dws) - 1, len(rec.bns) - 1))
    net = rec.conv('contraction_1x1_%d' % i, net, w_of(pw), 1, 1, (0, 0, 0, 0))
    net = bn_relu(bn_b, 'contraction_bn_%d' % i, net)
    feeds.append(('conv', len(rec.convs) - 1, len(rec.bns) - 1))
  feat = rnd(net.mean(dim=(2, 3)))
  logits = rec.conv('final_dense', feat[:, :, None, None], w_of(model.fc).reshape(1, 1, 1024, -1), 1, 1, (0, 0, 0, 0))
  logits = rnd(logits[:, :, 0, 0] + model.fc.bias.data.double())
  F.cross_entropy(logits, labels).backward()
  return rec, feeds


def test_mobilenet_v1_every_node_on_the_reference_tensors():
  """MobileNet-v1 (BASELINE config 5) at the benchmarked batch of 128 and 224 x 224, unsplit: kernel selection depends on
  the row counts, so the small-batch config test does not run these kernels.  Every conv node (the 3x3 / 2 stem on the
  tiny-C_in path, the 13 pointwise 1x1 convs, final_dense as a 1024 -> 1000 1x1 conv: 15), every depthwise node (13) and
  every batch-norm node (27, C = 32 over 1.6 M rows included) on the reference's tensors, and every statistics feed
  (stem -> initial_bn, depthwise -> bn_a, pointwise -> bn_b: 27) into the real batch norm."""
  rec, feeds = _record_mobilenet_v1(128, DEV)
  assert len(rec.convs) == 15 and len(rec.dws) == 13 and len(rec.bns) == 27 and len(feeds) == 27
  worst = 0.0
  for nd in rec.convs:
    worst = max(worst, check_conv_node(nd))
  for nd in rec.dws:
    worst = max(worst, check_dw_node(nd))
  for nd in rec.bns:
    worst = max(worst, check_bn_node(nd, sum_terms=True))
  for kind, si, bi in feeds:
    if kind == 'dw':
      check_dw_stats_feed(rec.dws[si], rec.bns[bi])
    else:
      check_stats_feed(rec.convs[si], rec.bns[bi])
  print('mobilenet_v1 chained: %d conv + %d depthwise + %d batch-norm nodes, %d statistics feeds, worst error / bound %.3f'
        % (len(rec.convs), len(rec.dws), len(rec.bns), len(feeds), worst))
  assert worst <= 1.0
